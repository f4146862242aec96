// bspline_kernels.hpp -- the device side of the B-spline calls (include/ife_hip.h): the recursive
// prefilter along the lines of every axis, the (order + 1)^3 gather and the 8-bit window.
//
// Prefilter.  A lane owns a line and runs, per pole, the causal start, the causal sweep, the
// anticausal start and the anticausal sweep, in place on doubles; the gain is applied where the
// first pole reads a sample for the first time (the same product, rounded on its own).  What
// depends on (z, N) only arrives in a BsAxis by value (bspline_plan.hpp).
//   Y and Z: neighbouring lanes own neighbouring x, so every access of a wave is one contiguous
//            piece of a row.
//   X:       a workgroup owns BSX_ROWS lines and moves them through an LDS tile of BSX_COLS
//            columns: the global accesses are whole 128-byte pieces of rows, the lanes sweep
//            their lines inside the tile (row pitch odd in doubles: no bank conflicts).
// Gather.  One workgroup per output y and group of BS_ZB output planes (grid capped, groups
// looped), x across lanes, templated on the order; the tables hold indices and weights, the kernel
// multiplies and adds, nested x, y, z, and reuses a source plane's sum from one output plane to
// the next.
// All offsets are 64-bit.  Double arithmetic, every operation rounded on its own
// (-ffp-contract=off).
#ifndef IFE_BSPLINE_KERNELS_HPP
#define IFE_BSPLINE_KERNELS_HPP

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "bspline_plan.hpp"

constexpr int BS_THREADS = 256;
constexpr int64_t BS_MAX_LINE_BLOCKS = 2048;    // line passes, conversion, window: the loop takes what lies beyond
constexpr int64_t BS_MAX_GATHER_BLOCKS = 1 << 12;  // gather: groups beyond it are taken by the group loop
constexpr int BS_ZB = 8;                           // gather: output planes per workgroup
constexpr int BSX_ROWS = BS_THREADS, BSX_COLS = 16, BSX_LD = BSX_COLS + 1;

// the source as doubles (orders 0 and 1: these are the coefficients)
template <typename TS>
__global__ __launch_bounds__(BS_THREADS) void bspline_convert_kernel(const TS *__restrict__ src,
                                                                     double *__restrict__ coef, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS_THREADS)
    coef[i] = (double)src[i];
}

// Lines of length n with element stride `stride`; line L starts at (L / inner) * outer + L % inner.
// Y pass: inner = nx, outer = nx * ny, stride = nx.  Z pass: inner = nx * ny, stride = nx * ny.
__global__ __launch_bounds__(BS_THREADS) void bspline_strided_kernel(double *__restrict__ c, const BsAxis ax,
                                                                     int64_t n, int64_t stride, int64_t inner,
                                                                     int64_t outer, int64_t lines) {
  for (int64_t line = (int64_t)blockIdx.x * BS_THREADS + threadIdx.x; line < lines;
       line += (int64_t)gridDim.x * BS_THREADS) {
    const int64_t o = line / inner;
    double *p = c + o * outer + (line - o * inner);
    for (int k = 0; k < ax.npoles; ++k) {
      const BsPole &pl = ax.pole[k];
      const double z = pl.z;
      const bool first_pole = k == 0;
      const double g = ax.gain;
      double s = first_pole ? p[0] * g : p[0];
      if (pl.full) {
        const double last = p[(n - 1) * stride];
        s = s + pl.first * (first_pole ? last * g : last);
      }
      for (int j = 1; j <= pl.count; ++j) {
        const double v = p[(int64_t)j * stride];
        s = s + pl.m[j - 1] * (first_pole ? v * g : v);
      }
      if (pl.full) s = s / pl.div;
      p[0] = s;
      double prev = s, prev2 = s;
      for (int64_t j = 1; j < n; ++j) {
        const double r = p[j * stride];
        const double v = (first_pole ? r * g : r) + z * prev;
        p[j * stride] = v;
        prev2 = prev;
        prev = v;
      }
      double nxt = pl.az * (z * prev2 + prev);
      p[(n - 1) * stride] = nxt;
      for (int64_t j = n - 2; j >= 0; --j) {
        const double v = z * (nxt - p[j * stride]);
        p[j * stride] = v;
        nxt = v;
      }
    }
  }
}

// tile <- columns [x0, x0 + BSX_COLS) of the workgroup's rows, and back; consecutive lanes take
// consecutive columns of a row, then the next row
__device__ __forceinline__ void bsx_load(double *tile, const double *c, int64_t r0, int nrows, int64_t x0, int64_t n) {
  for (int e = threadIdx.x; e < BSX_ROWS * BSX_COLS; e += BS_THREADS) {
    const int r = e / BSX_COLS, col = e - r * BSX_COLS;
    if (r < nrows && x0 + col < n) tile[r * BSX_LD + col] = c[(r0 + r) * n + x0 + col];
  }
}
__device__ __forceinline__ void bsx_store(const double *tile, double *c, int64_t r0, int nrows, int64_t x0,
                                          int64_t n) {
  for (int e = threadIdx.x; e < BSX_ROWS * BSX_COLS; e += BS_THREADS) {
    const int r = e / BSX_COLS, col = e - r * BSX_COLS;
    if (r < nrows && x0 + col < n) c[(r0 + r) * n + x0 + col] = tile[r * BSX_LD + col];
  }
}

// X pass: rows lines of length n, contiguous
__global__ __launch_bounds__(BS_THREADS) void bspline_x_kernel(double *__restrict__ c, const BsAxis ax, int64_t n,
                                                               int64_t rows) {
  __shared__ double tile[BSX_ROWS * BSX_LD];
  double *mine = tile + threadIdx.x * BSX_LD;
  for (int64_t r0 = (int64_t)blockIdx.x * BSX_ROWS; r0 < rows; r0 += (int64_t)gridDim.x * BSX_ROWS) {
    const int nrows = (int)(rows - r0 < BSX_ROWS ? rows - r0 : BSX_ROWS);
    const bool own = (int)threadIdx.x < nrows;  // every lane takes part in the tile moves and barriers
    for (int k = 0; k < ax.npoles; ++k) {
      const BsPole &pl = ax.pole[k];
      const double z = pl.z;
      const bool first_pole = k == 0;
      const double g = ax.gain;
      // causal start: c[0], c[N-1] where the sum is the full one, then c[1 .. count]
      double s = 0.0;
      for (int64_t x0 = 0; x0 <= pl.count; x0 += BSX_COLS) {
        bsx_load(tile, c, r0, nrows, x0, n);
        __syncthreads();
        if (own) {
          int j = 0;
          if (x0 == 0) {
            s = first_pole ? mine[0] * g : mine[0];
            if (pl.full) {
              const double last = c[(r0 + threadIdx.x) * n + (n - 1)];
              s = s + pl.first * (first_pole ? last * g : last);
            }
            j = 1;
          }
          for (; j < BSX_COLS && x0 + j <= pl.count; ++j) {
            const double v = mine[j];
            s = s + pl.m[x0 + j - 1] * (first_pole ? v * g : v);
          }
        }
        __syncthreads();
      }
      if (pl.full) s = s / pl.div;
      // causal sweep
      double prev = s, prev2 = s;
      for (int64_t x0 = 0; x0 < n; x0 += BSX_COLS) {
        bsx_load(tile, c, r0, nrows, x0, n);
        __syncthreads();
        if (own) {
          int j = 0;
          if (x0 == 0) {
            mine[0] = s;
            j = 1;
          }
          for (; j < BSX_COLS && x0 + j < n; ++j) {
            const double r = mine[j];
            const double v = (first_pole ? r * g : r) + z * prev;
            mine[j] = v;
            prev2 = prev;
            prev = v;
          }
        }
        __syncthreads();
        bsx_store(tile, c, r0, nrows, x0, n);
        __syncthreads();
      }
      // anticausal start and sweep, tiles from the last to the first
      double nxt = pl.az * (z * prev2 + prev);
      for (int64_t x0 = ((n - 1) / BSX_COLS) * BSX_COLS; x0 >= 0; x0 -= BSX_COLS) {
        bsx_load(tile, c, r0, nrows, x0, n);
        __syncthreads();
        if (own) {
          int j = (int)(n - 1 - x0 < BSX_COLS - 1 ? n - 1 - x0 : BSX_COLS - 1);
          if (x0 + j == n - 1) {
            mine[j] = nxt;
            --j;
          }
          for (; j >= 0; --j) {
            const double v = z * (nxt - mine[j]);
            mine[j] = v;
            nxt = v;
          }
        }
        __syncthreads();
        bsx_store(tile, c, r0, nrows, x0, n);
        __syncthreads();
      }
    }
  }
}

// one rounding; beyond +-FLT_MAX the value clamps (a NaN passes)
__device__ __forceinline__ float bs_to_out(double v, float) {
  return v > (double)FLT_MAX ? FLT_MAX : (v < -(double)FLT_MAX ? -FLT_MAX : (float)v);
}
__device__ __forceinline__ double bs_to_out(double v, double) { return v; }

// The gather.  W, I: K = ORDER + 1 weights / indices per output index, x entries first, then y,
// then z; E: the edge words in the same order.  kx, ky, kz: the taps an axis has (1 where the
// source axis has length 1, else K).  A workgroup takes one output y and BS_ZB consecutive output
// planes (groups = ny_t * ceil(nz_t / BS_ZB)): s(k), the sum over x and y taps of one SOURCE
// plane, depends on (x, y, source plane) only, so a lane keeps the K sums of the plane before and
// takes from them what the next output plane shares -- the same numbers, computed once.
template <typename TS, typename TO, int ORDER>
__global__ __launch_bounds__(BS_THREADS) void bspline_gather_kernel(
    const double *__restrict__ coef, const TS *__restrict__ src, TO *__restrict__ out, const double *__restrict__ W,
    const int32_t *__restrict__ I, const int32_t *__restrict__ E, int64_t nx_t, int64_t ny_t, int64_t nz_t,
    int64_t groups, int64_t nx_s, int64_t ny_s, int kx, int ky, int kz, int extrapolate, TO defv) {
  constexpr int K = ORDER + 1;
  const int64_t plane_s = nx_s * ny_s;
  for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int64_t zg = grp / ny_t, y = grp - zg * ny_t;
    const int64_t z0 = zg * BS_ZB, z1 = z0 + BS_ZB < nz_t ? z0 + BS_ZB : nz_t;
    const int64_t ty = nx_t + y;
    const int32_t ey = E[ty];
    double wy[K];
    int64_t oy[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      wy[k] = W[ty * K + k];
      oy[k] = (int64_t)I[ty * K + k] * nx_s;
    }
    for (int64_t x = threadIdx.x; x < nx_t; x += BS_THREADS) {
      const int32_t ex = E[x];
      const bool in_xy = bs_inside(ex) && bs_inside(ey);
      const int64_t edge_xy = (int64_t)bs_edge(ey) * nx_s + bs_edge(ex);
      double wx[K];
      int32_t ix[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        wx[i] = W[x * K + i];
        ix[i] = I[x * K + i];
      }
      double kept[K];     // s of the source planes kept_id, from the last inside output plane
      int32_t kept_id[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        kept[k] = 0.0;
        kept_id[k] = -1;
      }
      for (int64_t z = z0; z < z1; ++z) {
        const int64_t tz = nx_t + ny_t + z;
        const int32_t ez = E[tz];
        TO v = defv;
        if (in_xy && bs_inside(ez)) {
          double now[K];
          int32_t now_id[K];
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            now[k] = 0.0;
            now_id[k] = -1;
            if (k < kz) {
              const int32_t pz = I[tz * K + k];
              double s = 0.0;
              bool hit = false;
#pragma unroll
              for (int c = 0; c < K; ++c)
                if (kept_id[c] == pz) {
                  s = kept[c];
                  hit = true;
                }
              if (!hit) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                  if (j < ky) {
                    const double *p = coef + (int64_t)pz * plane_s + oy[j];
                    double r = wx[0] * p[ix[0]];
#pragma unroll
                    for (int i = 1; i < K; ++i)
                      if (i < kx) r = r + wx[i] * p[ix[i]];
                    s = j == 0 ? wy[0] * r : s + wy[j] * r;
                  }
                }
              }
              now[k] = s;
              now_id[k] = pz;
              const double wz = W[tz * K + k];
              acc = k == 0 ? wz * s : acc + wz * s;
            }
          }
#pragma unroll
          for (int k = 0; k < K; ++k) {
            kept[k] = now[k];
            kept_id[k] = now_id[k];
          }
          v = bs_to_out(acc, TO());
        } else if (extrapolate) {
          v = (TO)src[(int64_t)bs_edge(ez) * plane_s + edge_xy];
        }
        out[(z * ny_t + y) * nx_t + x] = v;
      }
    }
  }
}

// IntensityWindowingImageFilter to 8 bits and the mask; a NaN gives out_min
__global__ __launch_bounds__(BS_THREADS) void bspline_window_kernel(const double *__restrict__ src,
                                                                    const double *__restrict__ mask,
                                                                    uint8_t *__restrict__ out, int64_t n, double wmin,
                                                                    double wmax, double scale, double shift,
                                                                    uint8_t omin, uint8_t omax) {
  for (int64_t i = (int64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS_THREADS) {
    const double v = src[i];
    uint8_t r = omin;
    if (v > wmax) {
      r = omax;
    } else if (v >= wmin) {
      const double y = v * scale + shift;
      r = (uint8_t)(int)(y > 0.0 ? (y > 255.0 ? 255.0 : y) : 0.0);  // a NaN (scale overflowed) is 0
    }
    if (mask && !(mask[i] != 0.0)) r = 0;
    out[i] = r;
  }
}

#endif  // IFE_BSPLINE_KERNELS_HPP
