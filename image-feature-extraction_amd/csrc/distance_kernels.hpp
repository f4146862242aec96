// distance_kernels.hpp -- device side of SURVEY.md section 2 row 8: the signed Euclidean
// distance map of a mask (itk::SignedMaurerDistanceMapImageFilter as wired at
// include/ife/Statistics/ExpectedDistanceFromCenterToInterestPoint.h:16-19) and the masked
// mean of map * probability (:29-41).
//
// [ITK-upstream] restated, parity unpinned:
//   site      a foreground voxel with a background face neighbour inside the volume
//             (BinaryContourImageFilter, FullyConnected off)
//   D2(v)     min over sites c of ((hx(c)-hx(v))^2 + (hy(c)-hy(v))^2) + (hz(c)-hz(v))^2,
//             h(i) = (double)i * spacing, every operation rounded on its own; DBL_MAX
//             where the volume has no site
//   passes    x, y, z.  x: the contour test and the nearest site to the left and right of
//             every voxel of a row, from 64-bit ballots.  y, z: the lower envelope of the
//             parabolas g(j) + (h(j)-h(i))^2 of a line (Maurer, Qi, Raghavan 2003): a
//             stack of candidate sites built with the multiplication form of the "remove"
//             test (exact where the g are integers times a power of two), then one walk
//             along the line that evaluates the two candidates around the running
//             position.  Linear in the line length.
//
// All arithmetic is double compare / multiply / add at 8 bytes per voxel: HBM- and
// latency-bound, no MFMA.
#ifndef IFE_DISTANCE_KERNELS_HPP
#define IFE_DISTANCE_KERNELS_HPP

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

namespace ife {

// x pass: one wave per row; a row has at most EDT_MAX_SEGS ballots of 64 voxels
constexpr int EDT_MAX_SEGS = 512;
constexpr int64_t EDT_MAX_NX = (int64_t)64 * EDT_MAX_SEGS;
// y / z pass: one lane per line, this many waves in flight at most (sizes the stacks)
constexpr int EDT_MAX_LINE_BLOCKS = 2048;
constexpr int EDT_REDUCE_THREADS = 256;

// Row by row: the contour bits of 64 consecutive voxels are one ballot; a forward sweep leaves
// every segment's ballot and the last site before it in LDS, a backward sweep carries the first
// site after it and writes min(left^2, right^2) of the x distances (DBL_MAX: no site in the row).
template <typename TM>
__global__ __launch_bounds__(64) void edt_x_kernel(const TM *__restrict__ mask, double *__restrict__ out,
                                                   int64_t nx, int64_t ny, int64_t nz, double sx) {
  __shared__ uint64_t s_bits[EDT_MAX_SEGS];
  __shared__ int32_t s_left[EDT_MAX_SEGS];
  const int lane = threadIdx.x;
  const int nseg = (int)((nx + 63) / 64);
  const int64_t rows = ny * nz, plane = nx * ny;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t y = row % ny, z = row / ny;
    const TM *m = mask + row * nx;
    int last = -1;
    for (int s = 0; s < nseg; ++s) {
      const int64_t x = (int64_t)s * 64 + lane;
      bool site = false;
      if (x < nx && m[x] != 0) {  // neighbours outside the volume never make a site
        if (x > 0) site |= m[x - 1] == 0;
        if (x + 1 < nx) site |= m[x + 1] == 0;
        if (y > 0) site |= m[x - nx] == 0;
        if (y + 1 < ny) site |= m[x + nx] == 0;
        if (z > 0) site |= m[x - plane] == 0;
        if (z + 1 < nz) site |= m[x + plane] == 0;
      }
      const uint64_t bits = __ballot(site);
      if (lane == 0) {
        s_bits[s] = bits;
        s_left[s] = last;
      }
      if (bits) last = s * 64 + 63 - __builtin_clzll(bits);
    }
    __syncthreads();
    int next = -1;
    for (int s = nseg - 1; s >= 0; --s) {
      const uint64_t bits = s_bits[s];
      const uint64_t lo = bits & (~0ull >> (63 - lane));  // sites at or before this lane
      const uint64_t hi = bits & (~0ull << lane);         // sites at or after it
      const int l = lo ? s * 64 + 63 - __builtin_clzll(lo) : s_left[s];
      const int r = hi ? s * 64 + __builtin_ctzll(hi) : next;
      const int64_t x = (int64_t)s * 64 + lane;
      if (x < nx) {
        const double hx = (double)x * sx;
        double d = DBL_MAX;
        if (l >= 0) {
          const double t = (double)l * sx - hx;
          d = t * t;
        }
        if (r >= 0) {
          const double t = (double)r * sx - hx;
          const double e = t * t;
          d = e < d ? e : d;
        }
        out[row * nx + x] = d;
      }
      if (bits) next = s * 64 + __builtin_ctzll(bits);
    }
    __syncthreads();  // the next row overwrites the ballots
  }
}

struct EdtLines {
  int64_t nlines;  // lines of this axis, x-fastest
  int64_t inner;   // line -> first voxel: (line % inner) + (line / inner) * outer
  int64_t outer;
  int64_t stride;  // voxels between samples of a line
  int n;           // samples per line
  double spacing;
  double *ws_g;    // candidate stacks [k][slot]: value of the site's parabola at its vertex ...
  int32_t *ws_i;   // ... and its index along the line; slot = one lane of the grid
};

// Maurer's test: with u < v < w along the line, parabola v is nowhere below both u and w.
// c*gv - b*gu - a*gw - a*b*c > 0 with a = hv-hu, b = hw-hv, c = hw-hu: no division, exact for
// integer g and h (unit and power-of-two spacings) while c*g stays below 2^53.
__device__ __forceinline__ bool edt_remove(double gu, double gv, double gw, double hu, double hv, double hw) {
  const double a = hv - hu, b = hw - hv, c = hw - hu;
  return c * gv - b * gu - a * gw - a * b * c > 0.0;
}

// One lane per line, lanes adjacent in x (every access of a wave is to consecutive voxels).
// The line is consumed into the lane's candidate stack (the two top entries stay in registers)
// and rewritten in place: data[i] = min over j of data[j] + (h(j)-h(i))^2, DBL_MAX entries
// taking no part.  MODE 0: an inner pass.  MODE 1: the last pass, which stores
// out = +-(squared ? D2 : sqrt(D2)) instead.  MODE 2: the last pass of the expected distance:
// nothing is stored; the lane leaves sum over its foreground voxels of sqrt(D2) * prob, summed
// in line order, and their count in psum[line] / pcnt[line].
template <typename TM, int MODE>
__global__ __launch_bounds__(64) void edt_line_kernel(double *data, EdtLines a, const TM *__restrict__ mask,
                                                      int positive, int squared, double *out,
                                                      const double *__restrict__ prob, double *__restrict__ psum,
                                                      uint32_t *__restrict__ pcnt) {
  const int64_t nslots = (int64_t)gridDim.x * 64;
  const int64_t slot = (int64_t)blockIdx.x * 64 + threadIdx.x;
  double *sg = a.ws_g + slot;
  int32_t *si = a.ws_i + slot;
  const double sp = a.spacing;
  for (int64_t line = slot; line < a.nlines; line += nslots) {
    const int64_t base = line % a.inner + line / a.inner * a.outer;
    // build: candidates in line order; u = entry top-1, v = entry top
    int top = -1;
    double gu = 0.0, hu = 0.0, gv = 0.0, hv = 0.0;
    for (int i = 0; i < a.n; ++i) {
      const double gw = data[base + i * a.stride];
      if (gw == DBL_MAX) continue;
      const double hw = (double)i * sp;
      while (top >= 1 && edt_remove(gu, gv, gw, hu, hv, hw)) {
        --top;
        gv = gu;
        hv = hu;
        if (top >= 1) {
          gu = sg[(top - 1) * nslots];
          hu = (double)si[(top - 1) * nslots] * sp;
        }
      }
      ++top;
      gu = gv;
      hu = hv;
      gv = gw;
      hv = hw;
      sg[top * nslots] = gw;
      si[top * nslots] = i;
    }
    // query: the candidate under the running position and its successor
    const int ns = top + 1;
    int l = 0;
    double g0 = 0.0, h0 = 0.0, g1 = 0.0, h1 = 0.0;
    if (ns > 0) {
      g0 = sg[0];
      h0 = (double)si[0] * sp;
    }
    if (ns > 1) {
      g1 = sg[nslots];
      h1 = (double)si[nslots] * sp;
    }
    double sum = 0.0;
    uint32_t cnt = 0;
    for (int i = 0; i < a.n; ++i) {
      double d = DBL_MAX;
      if (ns > 0) {
        const double hi = (double)i * sp;
        const double t = h0 - hi;
        d = g0 + t * t;
        while (l + 1 < ns) {
          const double t1 = h1 - hi;
          const double d1 = g1 + t1 * t1;
          if (d <= d1) break;
          ++l;
          g0 = g1;
          h0 = h1;
          d = d1;
          if (l + 1 < ns) {
            g1 = sg[(l + 1) * nslots];
            h1 = (double)si[(l + 1) * nslots] * sp;
          }
        }
      }
      const int64_t v = base + i * a.stride;
      if (MODE == 0) {
        data[v] = d;
      } else {
        const bool fg = mask[v] != 0;
        if (MODE == 1) {
          const double r = squared ? d : sqrt(d);
          out[v] = fg == (positive != 0) ? r : -r;
        } else if (fg) {
          sum += sqrt(d) * prob[v];
          ++cnt;
        }
      }
    }
    if (MODE == 2) {
      psum[line] = sum;
      pcnt[line] = cnt;
    }
  }
}

// Fixed partition, fixed order: thread t adds the lines t, t + 256, ... in that order, the 256
// partial sums are combined by a binary tree.  result[0] = sum / n (0 when n == 0), the bits of
// result[1] hold n as int64.
__global__ __launch_bounds__(EDT_REDUCE_THREADS) void edt_reduce_kernel(const double *__restrict__ psum,
                                                                        const uint32_t *__restrict__ pcnt,
                                                                        int64_t nlines, double *__restrict__ result) {
  __shared__ double s_sum[EDT_REDUCE_THREADS];
  __shared__ unsigned long long s_cnt[EDT_REDUCE_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  unsigned long long c = 0;
  for (int64_t i = t; i < nlines; i += EDT_REDUCE_THREADS) {
    s += psum[i];
    c += pcnt[i];
  }
  s_sum[t] = s;
  s_cnt[t] = c;
  __syncthreads();
  for (int o = EDT_REDUCE_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) {
      s_sum[t] += s_sum[t + o];
      s_cnt[t] += s_cnt[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    const unsigned long long n = s_cnt[0];
    result[0] = n > 0 ? s_sum[0] / (double)n : 0.0;
    reinterpret_cast<unsigned long long *>(result)[1] = n;
  }
}

}  // namespace ife

#endif
