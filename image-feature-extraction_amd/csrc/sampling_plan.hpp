// sampling_plan.hpp -- the host side of ife_sample_positions, ife_random_rois and ife_extract_rois
// (include/ife_hip.h, DESIGN.md "Sampling"): the counter-based generator, the rank of a draw, the
// value sets and the argument checks.  Plain C++ (no HIP include), so that it compiles and is
// checked without a device: tests/csrc/sampling_plan_main.cpp prints what it computes for
// comparison with tests/sampling_oracle.py.  The generator and the rank are the functions the
// select kernel calls: under hipcc they are compiled for both sides.
#ifndef IFE_SAMPLING_PLAN_HPP
#define IFE_SAMPLING_PLAN_HPP

#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define SAMPLING_FN __host__ __device__ inline
#else
#define SAMPLING_FN inline
#endif

enum { SAMPLING_OK = 0, SAMPLING_E_ARG = 1, SAMPLING_E_SIZE = 2 };

constexpr int SAMPLING_MAX_VALUES = 32;
constexpr int64_t SAMPLING_MAX_OUTPUTS = (int64_t)1 << 36;  // sets * draws: 48 bytes each stay below 2^42
constexpr int64_t SAMPLING_MAX_BYTES = (int64_t)1 << 40;    // what ife_extract_rois writes

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11).
SAMPLING_FN void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;  // the increments after the tenth round are not used
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the high word of the 64 x 64 bit product
SAMPLING_FN uint64_t sampling_mulhi64(uint64_t a, uint64_t b) {
  const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
  const uint64_t mid = a1 * b0 + ((a0 * b0) >> 32);  // below 2^64: (2^32-1)^2 + 2^32 - 1
  const uint64_t mid2 = a0 * b1 + (uint32_t)mid;
  return a1 * b1 + (mid >> 32) + (mid2 >> 32);
}

// Rank of draw k of a set with n admissible voxels (n >= 1): floor(u * n / 2^64), u the first two
// output words of the generator at counter (k, stream), key seed.  `stream` is stream + j already.
SAMPLING_FN uint64_t sampling_rank(uint64_t seed, uint32_t stream, uint64_t k, uint64_t n) {
  const uint32_t ctr[4] = {(uint32_t)k, (uint32_t)(k >> 32), stream, 0u};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t o[4];
  philox4x32_10(ctr, key, o);
  return sampling_mulhi64((uint64_t)o[0] | ((uint64_t)o[1] << 32), n);
}

// The value sets of one call: n_values == 0 one set `mask != 0`; per_value == 0 one set `mask in
// values`; per_value == 1 n_values sets `mask == values[j]`.
struct SamplingSets {
  int n_sets, n_values, per_value;
  uint32_t values[SAMPLING_MAX_VALUES];
};

SAMPLING_FN bool sampling_member(const SamplingSets &s, int set, uint32_t v) {
  if (s.n_values == 0) return v != 0;
  if (s.per_value) return v == s.values[set];
  bool in = false;
  for (int i = 0; i < s.n_values; ++i) in = in || v == s.values[i];
  return in;
}

// The checks of the two sampling calls that need no device, in the order the header lists them.
// value_max: 255 or 65535.  size == NULL is {1, 1, 1}.  *msg: a static text.
inline int sampling_check(int value_max, const int *values, int n_values, int per_value, const int64_t *size,
                          int64_t n_draws, SamplingSets *sets, int64_t box[3], const char **msg) {
  if (n_values < 0 || n_values > SAMPLING_MAX_VALUES) {
    *msg = "n_values must lie in 0 .. 32";
    return SAMPLING_E_ARG;
  }
  if (n_values > 0 && !values) { *msg = "null pointer"; return SAMPLING_E_ARG; }
  if (per_value != 0 && per_value != 1) { *msg = "per_value must be 0 or 1"; return SAMPLING_E_ARG; }
  if (per_value && n_values == 0) { *msg = "per_value needs at least one value"; return SAMPLING_E_ARG; }
  sets->n_values = n_values;
  sets->per_value = per_value;
  sets->n_sets = per_value ? n_values : 1;
  for (int i = 0; i < SAMPLING_MAX_VALUES; ++i) sets->values[i] = 0;
  for (int i = 0; i < n_values; ++i) {
    if (values[i] < 0 || values[i] > value_max) {
      *msg = "a value is outside the range of the mask's type";
      return SAMPLING_E_ARG;
    }
    sets->values[i] = (uint32_t)values[i];
  }
  for (int a = 0; a < 3; ++a) {
    box[a] = size ? size[a] : 1;
    if (box[a] < 1) { *msg = "the box size must be at least 1 along every axis"; return SAMPLING_E_ARG; }
  }
  if (n_draws < 0) { *msg = "negative count"; return SAMPLING_E_ARG; }
  if (n_draws > SAMPLING_MAX_OUTPUTS / sets->n_sets) {
    *msg = "more than 2^36 draws over all sets";
    return SAMPLING_E_SIZE;
  }
  *msg = "";
  return SAMPLING_OK;
}

// Boxes of ife_extract_rois on the host: all of the size of the first, which is at least 1, and
// inside the volume n = {nx, ny, nz}.  Returns the first box that is not, or -1.
inline int64_t sampling_first_bad_box(const int64_t *rois, int64_t n_rois, const int64_t n[3]) {
  for (int64_t r = 0; r < n_rois; ++r) {
    const int64_t *q = rois + 6 * r;
    for (int a = 0; a < 3; ++a)
      if (q[3 + a] != rois[3 + a] || q[3 + a] < 1 || q[3 + a] > n[a] || q[a] < 0 || q[a] > n[a] - q[3 + a]) return r;
  }
  return -1;
}

// Bytes ife_extract_rois writes, or -1 beyond SAMPLING_MAX_BYTES.  size: of box 0, each in [1, 2^31).
inline int64_t sampling_gather_bytes(int64_t n_rois, const int64_t size[3], int elem_bytes) {
  int64_t count = elem_bytes;
  const int64_t f[4] = {size[0], size[1], size[2], n_rois};
  for (int a = 0; a < 4; ++a) {
    if (f[a] > 0 && count > SAMPLING_MAX_BYTES / f[a]) return -1;
    count *= f[a];
  }
  return count;
}

#endif  // IFE_SAMPLING_PLAN_HPP
