// coverage_plan.hpp -- the host side of ife_value_census_f32, ife_threshold_mask and
// ife_roi_coverage (include/ife_hip.h, DESIGN.md "Census and coverage"): the integer images of
// float bits the census and the threshold decide by, the word range and edge masks of a bit range
// of the one-bit-per-voxel planes, the tail word of such a plane and the argument checks.  Plain
// C++ (no HIP include), so that it compiles and is checked without a device:
// tests/csrc/coverage_plan_main.cpp prints what it computes.  The bit arithmetic is what the
// kernels call: under hipcc it is compiled for both sides.
#ifndef IFE_COVERAGE_PLAN_HPP
#define IFE_COVERAGE_PLAN_HPP

#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define COVERAGE_FN __host__ __device__ inline
#else
#define COVERAGE_FN inline
#endif

enum { COVERAGE_OK = 0, COVERAGE_E_ARG = 1, COVERAGE_E_SIZE = 2 };

constexpr int COVERAGE_MAX_ROUNDS = 64;
constexpr int64_t COVERAGE_MAX_VOXELS = 0xffffffffll;        // of a volume, as for sampling
constexpr int64_t CENSUS_MAX_VALUES = 0xffffffffll;          // what the header admits
constexpr int64_t CENSUS_MAX_SORTED = 0x7fffffffll;          // what the sort underneath takes
constexpr int64_t THRESHOLD_MAX_VALUES = (int64_t)1 << 40;

// ---- float bits ------------------------------------------------------------------------------------
COVERAGE_FN bool coverage_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

// -0 and +0 are one value of the census, reported as +0; every other bit pattern is its own value
COVERAGE_FN uint32_t census_canonical(uint32_t bits) { return bits == 0x80000000u ? 0u : bits; }

// The order-preserving integer image of a float that is no NaN: a < b as floats iff image(a) <
// image(b), and -0 and +0 share the image 0.  Denormals keep their order whatever the denormal mode
// of a float compare would be.
COVERAGE_FN int32_t coverage_order_image(uint32_t bits) {
  const int32_t mag = (int32_t)(bits & 0x7fffffffu);
  return (bits & 0x80000000u) ? -mag : mag;
}

COVERAGE_FN bool threshold_inside(uint32_t bits, int32_t low_image, int32_t high_image) {
  if (coverage_is_nan(bits)) return false;
  const int32_t v = coverage_order_image(bits);
  return low_image <= v && v <= high_image;
}

// ---- bit planes: bit (i & 31) of word (i >> 5) is voxel i -------------------------------------------
COVERAGE_FN int64_t coverage_words(int64_t nvox) { return (nvox + 31) >> 5; }

// the bits of the last word that are voxels; all of them where nvox is a multiple of 32
COVERAGE_FN uint32_t coverage_tail_mask(int64_t nvox) {
  const int r = (int)(nvox & 31);
  return r ? (1u << r) - 1u : 0xffffffffu;
}

// The bits [b0, b0 + n), n >= 1: words w0 .. w1; `first` are the bits of the range at or above its
// start in word w0, `last` the bits at or below its end in word w1.
struct CoverageBits {
  int64_t w0, w1;
  uint32_t first, last;
};

COVERAGE_FN CoverageBits coverage_bit_range(int64_t b0, int64_t n) {
  const int64_t b1 = b0 + n - 1;  // the last bit
  CoverageBits r;
  r.w0 = b0 >> 5;
  r.w1 = b1 >> 5;
  r.first = 0xffffffffu << (int)(b0 & 31);
  r.last = 0xffffffffu >> (31 - (int)(b1 & 31));
  return r;
}

// the bits of the range that lie in word w, w0 <= w <= w1
COVERAGE_FN uint32_t coverage_word_bits(const CoverageBits &r, int64_t w) {
  return (w == r.w0 ? r.first : 0xffffffffu) & (w == r.w1 ? r.last : 0xffffffffu);
}

// A box {x0, y0, z0, sx, sy, sz} of a volume n = {nx, ny, nz}: every size at least 1 and the box
// inside.  Nothing overflows: no sum of two arguments is formed.
COVERAGE_FN bool coverage_box_ok(const int64_t *q, const int64_t n[3]) {
  for (int a = 0; a < 3; ++a)
    if (q[3 + a] < 1 || q[3 + a] > n[a] || q[a] < 0 || q[a] > n[a] - q[3 + a]) return false;
  return true;
}

// the first box that is not, or -1
inline int64_t coverage_first_bad_box(const int64_t *rois, int64_t n_rois, const int64_t n[3]) {
  for (int64_t r = 0; r < n_rois; ++r)
    if (!coverage_box_ok(rois + 6 * r, n)) return r;
  return -1;
}

// ---- the argument checks that need no device, in the order the header lists them; *msg: a static text
inline int census_check(bool has_values, int64_t n, bool has_uniq, bool has_counts, int64_t capacity,
                        bool has_n_unique, bool has_n_nan, const char **msg) {
  *msg = "null pointer";
  if (!has_values || !has_n_unique || !has_n_nan) return COVERAGE_E_ARG;
  if (n <= 0) { *msg = "the element count must be positive"; return COVERAGE_E_ARG; }
  if (capacity < 0) { *msg = "negative capacity"; return COVERAGE_E_ARG; }
  // the outputs may be missing together where nothing is to be written
  if (has_uniq != has_counts || (capacity > 0 && !has_uniq)) return COVERAGE_E_ARG;
  if (n > CENSUS_MAX_VALUES) { *msg = "more than 2^32-1 elements"; return COVERAGE_E_SIZE; }
  if (n > CENSUS_MAX_SORTED) { *msg = "the sort takes at most 2^31-1 elements"; return COVERAGE_E_SIZE; }
  *msg = "";
  return COVERAGE_OK;
}

inline int threshold_check(bool has_image, bool has_mask, int64_t n, uint32_t low_bits, uint32_t high_bits,
                           const char **msg) {
  if (!has_image || !has_mask) { *msg = "null pointer"; return COVERAGE_E_ARG; }
  if (coverage_is_nan(low_bits) || coverage_is_nan(high_bits)) {
    *msg = "a threshold is not a number";
    return COVERAGE_E_ARG;
  }
  if (coverage_order_image(low_bits) > coverage_order_image(high_bits)) {
    *msg = "Lower threshold cannot be greater than upper threshold.";
    return COVERAGE_E_ARG;
  }
  if (n <= 0 || n > THRESHOLD_MAX_VALUES) {
    *msg = "the element count must lie in 1 .. 2^40";
    return COVERAGE_E_SIZE;
  }
  *msg = "";
  return COVERAGE_OK;
}

// round_ends: non-decreasing, each in 0 .. n_rois, 1 .. 64 of them
inline int coverage_check_rounds(const int64_t *round_ends, int n_rounds, int64_t n_rois, const char **msg) {
  if (n_rounds < 1 || n_rounds > COVERAGE_MAX_ROUNDS) {
    *msg = "n_rounds must lie in 1 .. 64";
    return COVERAGE_E_ARG;
  }
  if (!round_ends) { *msg = "null pointer"; return COVERAGE_E_ARG; }
  if (n_rois < 0) { *msg = "negative count"; return COVERAGE_E_ARG; }
  int64_t prev = 0;
  for (int r = 0; r < n_rounds; ++r) {
    if (round_ends[r] < prev) {
      *msg = r ? "round_ends decreases" : "a round end is negative";
      return COVERAGE_E_ARG;
    }
    if (round_ends[r] > n_rois) { *msg = "a round end lies beyond n_rois"; return COVERAGE_E_ARG; }
    prev = round_ends[r];
  }
  *msg = "";
  return COVERAGE_OK;
}

// the voxel count of a volume of positive axis lengths below 2^31 each, or -1 beyond 2^32-1
inline int64_t coverage_voxels(int64_t nx, int64_t ny, int64_t nz) {
  const int64_t plane = nx * ny;
  if (plane > COVERAGE_MAX_VOXELS || nz > COVERAGE_MAX_VOXELS / plane) return -1;
  return plane * nz;
}

#endif  // IFE_COVERAGE_PLAN_HPP
