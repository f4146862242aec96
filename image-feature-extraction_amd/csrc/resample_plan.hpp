// resample_plan.hpp -- the axis tables of ife_resample (include/ife_hip.h, DESIGN.md "Resampling").
// Plain host C++ (no HIP include): the transform is an axis-aligned translation, so where an
// output voxel lands in the source factors per axis, and everything that needs a division is
// done here once per output index, O(nx + ny + nz), in the arithmetic the header states.  The
// kernel (resample_kernels.hpp) reads the packed entries; tests/csrc/resample_plan_main.cpp
// prints them for comparison with tests/resample_oracle.py.
#ifndef IFE_RESAMPLE_PLAN_HPP
#define IFE_RESAMPLE_PLAN_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define IFE_RS_HD __host__ __device__
#else
#define IFE_RS_HD
#endif

// One output index of one axis, 16 bytes (one load per lane along x).
//   b    -1: outside; else the lower source index, 0 <= b <= n_s - 1
//   near the nearest source index, 0 <= near <= n_s - 1; stored as ~near (negative) where the
//        axis is skipped, i.e. the linear value is the one at b and b + 1 is not read
//   t    c - b, the weight of b + 1
struct ResampleEntry {
  double t;
  int32_t b;
  int32_t near_skip;
};
static_assert(sizeof(ResampleEntry) == 16, "packed table entry");

IFE_RS_HD inline bool rs_inside(const ResampleEntry &e) { return e.b >= 0; }
IFE_RS_HD inline bool rs_skip(const ResampleEntry &e) { return e.near_skip < 0; }
IFE_RS_HD inline int32_t rs_near(const ResampleEntry &e) { return e.near_skip < 0 ? ~e.near_skip : e.near_skip; }

// The entry of output index i: n_s, s_s, o_s describe the source axis, s_t and o_t the output
// axis, tr is the translation.  Every operation rounds on its own (the build has contraction
// off).  No value is converted to an integer unless it is inside, so that huge, infinite and NaN
// coordinates are "outside" and nothing else.
inline ResampleEntry resample_entry(int64_t i, int64_t n_s, double s_s, double o_s, double s_t, double o_t,
                                    double tr) {
  const double p = o_t + (double)i * s_t;
  const double q = p + tr;
  const double c = (q - o_s) / s_s;
  const bool inside = (c >= -0.5) && (c < (double)(n_s - 1) + 0.5);
  ResampleEntry e{0.0, -1, 0};
  if (!inside) return e;
  int64_t b = (int64_t)std::floor(c);
  if (b < 0) b = 0;  // c in [-0.5, 0): b = 0 and t < 0
  const double t = c - (double)b;
  const bool skip = (t <= 0.0) || (b + 1 > n_s - 1);
  // the min is a bound, not cosmetics: n_s = 1, c = 0.49999999999999994 gives c + 0.5 == 1.0
  int64_t near = (int64_t)std::floor(c + 0.5);
  if (near > n_s - 1) near = n_s - 1;
  e.t = t;
  e.b = (int32_t)b;
  e.near_skip = skip ? ~(int32_t)near : (int32_t)near;
  return e;
}

// n_t entries of one axis into `out`
inline void resample_axis_table(int64_t n_t, int64_t n_s, double s_s, double o_s, double s_t, double o_t,
                                double tr, ResampleEntry *out) {
  for (int64_t i = 0; i < n_t; ++i) out[i] = resample_entry(i, n_s, s_s, o_s, s_t, o_t, tr);
}

#endif  // IFE_RESAMPLE_PLAN_HPP
