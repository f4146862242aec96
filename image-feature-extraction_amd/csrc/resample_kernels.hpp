// resample_kernels.hpp -- the gather of ife_resample / ife_resample_f64 (include/ife_hip.h).
// One workgroup per output row (grid capped, rows looped): x runs across lanes, so every store of
// a wave writes one contiguous piece of the row; the y and z table entries of the row are the
// same for the whole workgroup, the x entry is one 16-byte load per lane (resample_plan.hpp).
// The eight source values of a voxel come from two rows of two planes; neighbouring output rows
// and planes reread them out of L2.  All offsets are 64-bit.  Double arithmetic, every operation
// rounded on its own (-ffp-contract=off), one rounding to the output type at the end.
#ifndef IFE_RESAMPLE_KERNELS_HPP
#define IFE_RESAMPLE_KERNELS_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "resample_plan.hpp"

constexpr int RS_THREADS = 256;
constexpr int64_t RS_MAX_BLOCKS = 1 << 20;  // rows beyond it are taken by the row loop

// L of the definition: a select, never a multiplication by zero -- a skipped axis hands `a` on
// untouched (an infinity, a NaN payload)
__device__ __forceinline__ double rs_lerp(double a, double b, double t, bool skip) {
  return skip ? a : a + (b - a) * t;
}

// INTERP 0: linear, 1: nearest.  rows = ny_t * nz_t.
template <typename TS, typename TO, int INTERP>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    const TS *__restrict__ src, TO *__restrict__ out, const ResampleEntry *__restrict__ tx,
    const ResampleEntry *__restrict__ ty, const ResampleEntry *__restrict__ tz, int64_t nx_t, int64_t ny_t,
    int64_t rows, int64_t nx_s, int64_t ny_s, TO defv) {
  const int64_t plane_s = nx_s * ny_s;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t z = row / ny_t, y = row - z * ny_t;
    const ResampleEntry ey = ty[y], ez = tz[z];
    const bool in_yz = rs_inside(ey) && rs_inside(ez);
    TO *orow = out + row * nx_t;
    // base of the row pair: (0, by, bz) or, for nearest, (0, near_y, near_z)
    int64_t base = 0, dy = 0, dz = 0;
    if (in_yz) {
      if (INTERP == 0) {
        base = (int64_t)ez.b * plane_s + (int64_t)ey.b * nx_s;
        dy = rs_skip(ey) ? 0 : nx_s;  // a skipped axis reads its own voxel again, not the neighbour
        dz = rs_skip(ez) ? 0 : plane_s;
      } else {
        base = (int64_t)rs_near(ez) * plane_s + (int64_t)rs_near(ey) * nx_s;
      }
    }
    for (int64_t x = threadIdx.x; x < nx_t; x += RS_THREADS) {
      TO v = defv;
      if (in_yz) {
        const ResampleEntry ex = tx[x];
        if (rs_inside(ex)) {
          if (INTERP == 0) {
            const bool sx = rs_skip(ex), sy = rs_skip(ey), sz = rs_skip(ez);
            const TS *p = src + base + ex.b;
            const int64_t dx = sx ? 0 : 1;
            const double v000 = (double)p[0], v100 = (double)p[dx];
            const double v010 = (double)p[dy], v110 = (double)p[dy + dx];
            const double v001 = (double)p[dz], v101 = (double)p[dz + dx];
            const double v011 = (double)p[dz + dy], v111 = (double)p[dz + dy + dx];
            const double vx00 = rs_lerp(v000, v100, ex.t, sx);
            const double vx10 = rs_lerp(v010, v110, ex.t, sx);
            const double vx01 = rs_lerp(v001, v101, ex.t, sx);
            const double vx11 = rs_lerp(v011, v111, ex.t, sx);
            const double vxy0 = rs_lerp(vx00, vx10, ey.t, sy);
            const double vxy1 = rs_lerp(vx01, vx11, ey.t, sy);
            v = (TO)rs_lerp(vxy0, vxy1, ez.t, sz);
          } else {
            v = (TO)src[base + rs_near(ex)];
          }
        }
      }
      orow[x] = v;
    }
  }
}

#endif  // IFE_RESAMPLE_KERNELS_HPP
