// region_plan.hpp -- the host side of ife_extract_region (include/ife_hip.h, DESIGN.md "Regions"):
// the argument checks, the split of every output axis into [pad | copy | pad] and the geometry of
// a cropped or padded output.  Plain host C++ (no HIP include), so that it compiles and is checked
// without a device: tests/csrc/region_plan_main.cpp prints what it computes for comparison with
// tests/region_oracle.py.
#ifndef IFE_REGION_PLAN_HPP
#define IFE_REGION_PLAN_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>

enum { REGION_OK = 0, REGION_E_ARG = 1, REGION_E_SIZE = 2 };

constexpr int64_t REGION_MAX_BYTES = (int64_t)1 << 40;

// One output axis: output indices [0, lo) are pad, [lo, lo + n) are copied, the rest (hi) is pad.
// Output index lo + k reads source index src0 + k * step, step = +1 or -1 (flip).
struct RegionAxis {
  int64_t lo, n, hi;
  int64_t src0;
  int step;
};

// The split of one axis: the output has `size` elements, element i reads source index
// idx + (flip ? size - 1 - i : i) of a source axis of n_src elements.  idx is any int64: nothing
// here overflows (idx + size is formed only where idx is inside (-size, n_src)).
inline RegionAxis region_axis(int64_t idx, int64_t size, int64_t n_src, bool flip) {
  RegionAxis a{size, 0, 0, 0, flip ? -1 : 1};
  if (idx >= n_src || idx <= -size) return a;  // wholly outside: all pad, no source address
  const int64_t s_lo = idx < 0 ? 0 : idx;                              // first source index read
  const int64_t s_hi = idx + size < n_src ? idx + size : n_src;        // one past the last
  a.n = s_hi - s_lo;
  const int64_t before = s_lo - idx, after = idx + size - s_hi;  // pad in the order of the source
  a.lo = flip ? after : before;
  a.hi = flip ? before : after;
  a.src0 = flip ? s_hi - 1 : s_lo;
  return a;
}

struct RegionPlan {
  RegionAxis ax[3];
  bool inside;    // no pad anywhere
  bool all_pad;   // no source element is read
};

// The checks of ife_extract_region that need no device, in the order the header lists them.
// *msg: a static text.  n_src: the source's {nx, ny, nz}, each in [1, 2^31).
inline int region_check(int elem_bytes, const int64_t n_src[3], const int64_t *region, int flip, bool has_pad,
                        RegionPlan *plan, const char **msg) {
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) {
    *msg = "elem_bytes must be 1, 2, 4 or 8";
    return REGION_E_ARG;
  }
  if (!region) { *msg = "null pointer"; return REGION_E_ARG; }
  if (flip < 0 || flip > 7) { *msg = "flip must be 0 .. 7 (bit a flips axis a)"; return REGION_E_ARG; }
  for (int a = 0; a < 3; ++a)
    if (region[3 + a] < 1) { *msg = "the region's size must be at least 1 on every axis"; return REGION_E_ARG; }
  int64_t count = elem_bytes;  // bytes, kept at or below 2^40 after every factor
  for (int a = 0; a < 3; ++a) {
    if (region[3 + a] > REGION_MAX_BYTES / count) {
      *msg = "the region holds more than 2^40 bytes";
      return REGION_E_SIZE;
    }
    count *= region[3 + a];
  }
  plan->inside = true;
  plan->all_pad = false;
  for (int a = 0; a < 3; ++a) {
    plan->ax[a] = region_axis(region[a], region[3 + a], n_src[a], (flip >> a) & 1);
    if (plan->ax[a].n != region[3 + a]) plan->inside = false;
    if (plan->ax[a].n == 0) plan->all_pad = true;
  }
  if (!plan->inside && !has_pad) {
    *msg = "the region reaches outside the source and pad_value is null";
    return REGION_E_ARG;
  }
  *msg = "";
  return REGION_OK;
}

// ---- geometry of a cropped or padded output (direction ignored, as everywhere in the mirror) ----
// origin + index o spacing
inline void region_shift_origin(const double origin[3], const double spacing[3], const int64_t index[3],
                                double out[3]) {
  for (int a = 0; a < 3; ++a) out[a] = origin[a] + (double)index[a] * spacing[a];
}

// NIfTI sform: srow[r][3] += sum_a srow[r][a] * index[a], in double, rounded to float once
inline void region_shift_srow(float srow[3][4], const int64_t index[3]) {
  for (int r = 0; r < 3; ++r) {
    double t = (double)srow[r][3];
    for (int a = 0; a < 3; ++a) t += (double)srow[r][a] * (double)index[a];
    srow[r][3] = (float)t;
  }
}

// NIfTI qform: the rotation of the quaternion (b, c, d; a = sqrt(1 - b^2 - c^2 - d^2), the
// NIfTI-1 normalisation where that is not positive), qfac on the z column, applied to
// pixdim o index; in double, rounded to float once.
inline void region_shift_qoffset(const float quatern[3], float qfac, const double pixdim[3], const int64_t index[3],
                                 float qoffset[3]) {
  double b = quatern[0], c = quatern[1], d = quatern[2], a = 1.0 - (b * b + c * c + d * d);
  if (a < 1e-7) {
    a = 1.0 / std::sqrt(b * b + c * c + d * d);
    b *= a; c *= a; d *= a;
    a = 0.0;
  } else {
    a = std::sqrt(a);
  }
  const double R[3][3] = {{a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c},
                          {2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b},
                          {2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b}};
  const double v[3] = {pixdim[0] * (double)index[0], pixdim[1] * (double)index[1],
                       (qfac < 0.0f ? -1.0 : 1.0) * pixdim[2] * (double)index[2]};
  for (int r = 0; r < 3; ++r)
    qoffset[r] = (float)((double)qoffset[r] + (R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2]));
}

// MetaImage: Offset += D * (spacing o index); the file's TransformMatrix lists the direction of
// image axis a as its a-th triple, i.e. m[3 * a + r] is D[r][a].
inline void region_shift_mhd_offset(const double m[9], const double spacing[3], const int64_t index[3],
                                    double offset[3]) {
  for (int r = 0; r < 3; ++r) {
    double t = 0.0;
    for (int a = 0; a < 3; ++a) t += m[3 * a + r] * (spacing[a] * (double)index[a]);
    offset[r] += t;
  }
}

#endif  // IFE_REGION_PLAN_HPP
