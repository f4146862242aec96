// dense_kernels.hpp -- device side of the dense bag (tools/MakeBagDense.cxx:239-250): one
// region per mask voxel whose box fits the volume (include/ife/ROI/DenseROIGenerator.hxx:24-46),
// every region binned as tools/MakeBag.cxx:405-472 bins a box.
//
// All boxes of a dense bag have one size, so the count of bin b in the box around voxel v is the
// 3-D box sum of the indicator "v is in the mask and falls into bin b".  Box sums are separable:
//
//   centres  one flag per voxel (generating mask != 0 and the box fits) and, per 64-voxel row
//            segment, the number of flags; the exclusive scan of those numbers (chunk_sum /
//            scan_chunks / chunk_scan of stats_kernels.hpp) numbers the regions in raster order
//   codes    per component one byte per voxel: the bin (the search of roi_histogram_kernel), or
//            DENSE_OUTSIDE where the counting mask is 0
//   x pass   a wave per row segment, lanes along x: per bin the ballot of `code == bin` over the
//            segment and its neighbours, the window count is a popcount of the window's bits
//   y pass   lanes along x, marching y: running sum (add the row that enters, subtract the one
//            that leaves), one byte in, two bytes out
//   z pass   the same along z, two bytes in; stores nothing but the final counts, at the centres,
//            straight into counts[row][component][bin] (or, for the stream of row blocks, into a
//            planar block buffer [column][row in block], so that a wave's stores are one run)
//   freq     stream only: the planar block to the row-major block that goes to the host,
//            transposed through LDS, as counts or as DenseHistogram::getFrequencies forms them
//
// The x and y passes work plane by plane, so a block of centre planes [zc0, zc1) runs them on a
// DenseGeom whose nz is the block's plane count (zc1 - zc0 + sz - 1) with pointers offset to plane
// zc0 - hz; the z pass takes the flags and segment bases offset likewise and the block's first row.
//
// Work per voxel, component and bin is constant: it does not grow with the box.  Everything is
// integer counting and every output word has exactly one writer, so the result does not depend on
// the order of execution and equals the per-box path bit for bit.
#ifndef IFE_DENSE_KERNELS_HPP
#define IFE_DENSE_KERNELS_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stats_kernels.hpp"

namespace ife {

constexpr int DENSE_MAX_EDGES = 254;  // bins 0..254 in one byte, 255 is "not in the mask"
constexpr int DENSE_OUTSIDE = 255;
// counter widths: one byte after x, two after y, four after z
constexpr int64_t DENSE_MAX_SX = 255, DENSE_MAX_SXY = 65535, DENSE_MAX_SXYZ = 0xffffffffll;
constexpr int DENSE_X_PIECES = (64 + (int)DENSE_MAX_SX - 1 + 63) / 64;  // 64-voxel pieces a window row spans

struct DenseGeom {
  int64_t nx, ny, nz, nvox;
  int sx, sy, sz;  // box size
  int hx, hy, hz;  // centre to box corner: size / 2 (integer division, DenseROIGenerator.hxx:35-40)
  int gx;          // 64-voxel segments per row
};

__device__ __forceinline__ bool dense_fits(const DenseGeom &g, int64_t x, int64_t y, int64_t z) {
  return x >= g.hx && x - g.hx + g.sx <= g.nx && y >= g.hy && y - g.hy + g.sy <= g.ny && z >= g.hz &&
         z - g.hz + g.sz <= g.nz;
}

// One wave per row segment s = bx + gx * row: flag[i] = voxel i is a centre, counts[s] = the
// segment's number of centres.
template <typename TM>
__global__ __launch_bounds__(256) void dense_centre_kernel(const TM *__restrict__ gen,
                                                           uint8_t *__restrict__ flag,
                                                           uint32_t *__restrict__ counts, DenseGeom g,
                                                           int64_t nseg) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = wave0; s < nseg; s += nwaves) {
    const int64_t row = s / g.gx;
    const int64_t x = (s % g.gx) * 64 + lane;
    bool on = false;
    if (x < g.nx) {
      const int64_t i = row * g.nx + x;
      on = gen[i] != 0 && dense_fits(g, x, row % g.ny, row / g.ny);
      flag[i] = on ? 1 : 0;
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(on);
    if (lane == 0) counts[s] = (uint32_t)__popcll(m);
  }
}

// DenseROIGenerator<TMask>::generate: box {x0, y0, z0, sx, sy, sz} of every centre, at the
// centre's number (seg_base: exclusive scan of the segment counts).
__global__ __launch_bounds__(256) void dense_boxes_kernel(const uint8_t *__restrict__ flag,
                                                          const uint32_t *__restrict__ seg_base,
                                                          int64_t *__restrict__ rois, DenseGeom g,
                                                          int64_t nseg) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = wave0; s < nseg; s += nwaves) {
    const int64_t row = s / g.gx;
    const int64_t x = (s % g.gx) * 64 + lane;
    const bool on = x < g.nx && flag[row * g.nx + x] != 0;
    const uint64_t m = __builtin_amdgcn_ballot_w64(on);
    if (on) {
      int64_t *q = rois + 6 * ((int64_t)seg_base[s] + lanes_below(m));
      q[0] = x - g.hx; q[1] = row % g.ny - g.hy; q[2] = row / g.ny - g.hz;
      q[3] = g.sx; q[4] = g.sy; q[5] = g.sz;
    }
  }
}

// DenseHistogram bin of v: the lower bound over the nedges ascending edges e.
__device__ __forceinline__ int dense_bin(const float *e, int nedges, float v) {
  int lo = 0, hi = nedges;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Bin codes of components [c0, c0 + gridDim.y) of one feature volume: code[c][i] = DenseHistogram
// bin of the component value (lower bound over the edges; a NaN goes to bin 0 because
// `e[mid] < v` is false throughout, as in roi_histogram_kernel), DENSE_OUTSIDE where mask == 0.
template <typename TM>
__global__ __launch_bounds__(256) void dense_code_kernel(const float *__restrict__ feat,
                                                         const TM *__restrict__ mask,
                                                         const float *__restrict__ edges,
                                                         uint8_t *__restrict__ code, int64_t nvox,
                                                         int64_t comp_stride, int64_t vox_stride, int c0,
                                                         int nedges) {
  __shared__ float e[DENSE_MAX_EDGES];
  const int c = blockIdx.y;
  for (int i = threadIdx.x; i < nedges; i += blockDim.x) e[i] = edges[(int64_t)(c0 + c) * nedges + i];
  __syncthreads();
  const float *f = feat + (int64_t)(c0 + c) * comp_stride;
  uint8_t *out = code + (int64_t)c * nvox;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox;
       i += (int64_t)gridDim.x * blockDim.x) {
    int lo = DENSE_OUTSIDE;
    if (mask[i] != 0) lo = dense_bin(e, nedges, f[i * vox_stride]);
    out[i] = (uint8_t)lo;
  }
}

// x pass over planes (component c of the group, bin b0 + b): xs[c * nbins + b][i] = number of
// voxels of the window [x - hx, x - hx + sx) of i's row with code == b0 + b; 0 where the window
// leaves the row.  One wave per (row segment, component): the codes of the segment and of the
// pieces the windows reach into are read once, per bin a ballot per piece and a popcount of the
// window's bits in it.  nwork = gx * ny * nz * ncomp.  code_stride: bytes from one component's
// codes to the next (g.nvox, or the whole volume's where g is a block of its planes).
__global__ __launch_bounds__(256) void dense_box_x_kernel(const uint8_t *__restrict__ code,
                                                          int64_t code_stride, uint8_t *__restrict__ xs,
                                                          DenseGeom g, int b0, int nbins, int64_t nwork) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t nrows = g.ny * g.nz;
  const int npieces = (64 + g.sx - 1 + 63) / 64;
  // the bits of piece j that belong to this lane's window: loaded voxel k = 64 j + bit sits at
  // x0 - hx + k, the window of lane l covers k in [l, l + sx)
  uint64_t wbits[DENSE_X_PIECES];
#pragma unroll
  for (int j = 0; j < DENSE_X_PIECES; ++j) {
    const int lo = min(max(lane - 64 * j, 0), 64), hi = min(max(lane + g.sx - 64 * j, 0), 64);
    const uint64_t below_hi = hi >= 64 ? ~0ull : (1ull << hi) - 1;
    wbits[j] = hi > lo ? below_hi & ~((1ull << lo) - 1) : 0ull;
  }
  for (int64_t w = wave0; w < nwork; w += nwaves) {
    const int64_t seg = w % g.gx, t = w / g.gx, row = t % nrows, c = t / nrows;
    const int64_t x = seg * 64 + lane, p0 = seg * 64 - g.hx;
    const uint8_t *src = code + c * code_stride + row * g.nx;
    int k[DENSE_X_PIECES];
#pragma unroll
    for (int j = 0; j < DENSE_X_PIECES; ++j) {
      const int64_t p = p0 + 64 * j + lane;
      k[j] = (j < npieces && p >= 0 && p < g.nx) ? (int)src[p] : DENSE_OUTSIDE;
    }
    const bool fits = x >= g.hx && x - g.hx + g.sx <= g.nx;
    uint8_t *dst = xs + c * nbins * g.nvox + row * g.nx + x;
    for (int b = 0; b < nbins; ++b) {
      int n = 0;
#pragma unroll
      for (int j = 0; j < DENSE_X_PIECES; ++j)
        if (j < npieces) n += __popcll(__builtin_amdgcn_ballot_w64(k[j] == b0 + b) & wbits[j]);
      if (x < g.nx) dst[(int64_t)b * g.nvox] = (uint8_t)(fits ? n : 0);
    }
  }
}

// y pass: ys[p][x, y, z] = sum of xs[p][x, yy, z] over the window yy in [y - hy, y - hy + sy), for
// the ny - sy + 1 rows y whose window fits.  Lanes along x; a wave marches `chunk` output rows of
// one (segment, z, plane).  nwork = gx * nz * nchunks * nplanes.
__global__ __launch_bounds__(256) void dense_box_y_kernel(const uint8_t *__restrict__ xs,
                                                          uint16_t *__restrict__ ys, DenseGeom g,
                                                          int chunk, int nchunks, int64_t nwork) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t nout = g.ny - g.sy + 1;
  for (int64_t w = wave0; w < nwork; w += nwaves) {
    int64_t t = w;
    const int64_t seg = t % g.gx; t /= g.gx;
    const int64_t z = t % g.nz; t /= g.nz;
    const int64_t ch = t % nchunks, p = t / nchunks;
    const int64_t x = seg * 64 + lane;
    if (x >= g.nx) continue;
    const int64_t o0 = ch * chunk, o1 = min(o0 + chunk, nout);
    const int64_t base = p * g.nvox + z * g.nx * g.ny + x;
    const uint8_t *in = xs + base;
    uint16_t *out = ys + base;
    uint32_t s = 0;
    for (int64_t y = o0; y < o0 + g.sy - 1; ++y) s += in[y * g.nx];
#pragma unroll 4
    for (int64_t o = o0; o < o1; ++o) {
      s += in[(o + g.sy - 1) * g.nx];
      out[(o + g.hy) * g.nx] = (uint16_t)s;
      s -= in[o * g.nx];
    }
  }
}

// z pass of plane p = c * nbins + b: the running sum of ys[p] along z is the count of bin b0 + b
// of component c in the box around (x, y, z); it is stored only where flag says centre, at
// counts[(number - row0) * row_stride + (col0 + c * nb + b) * col_stride]: row-major rows with
// (row_words, 1), a planar block [column][row in block] with (1, rows the block buffer holds).
// row0: the number of the first region of g (0 for a whole volume).  Lanes along x, a wave marches
// `chunk` planes of one (segment, y, plane) for the ny - sy + 1 rows y whose window fits.
// nwork = gx * (ny - sy + 1) * nchunks * nplanes.
__global__ __launch_bounds__(256) void dense_box_z_kernel(const uint16_t *__restrict__ ys,
                                                          const uint8_t *__restrict__ flag,
                                                          const uint32_t *__restrict__ seg_base,
                                                          uint32_t *__restrict__ counts, DenseGeom g,
                                                          int nbins, int nb, int64_t row0,
                                                          int64_t row_stride, int64_t col_stride,
                                                          int64_t col0, int chunk, int nchunks,
                                                          int64_t nwork) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t nyv = g.ny - g.sy + 1, nout = g.nz - g.sz + 1, plane = g.nx * g.ny;
  for (int64_t w = wave0; w < nwork; w += nwaves) {
    int64_t t = w;
    const int64_t seg = t % g.gx; t /= g.gx;
    const int64_t y = t % nyv + g.hy; t /= nyv;
    const int64_t ch = t % nchunks, p = t / nchunks;
    const bool live = seg * 64 + lane < g.nx;
    const int64_t x = live ? seg * 64 + lane : g.nx - 1;  // idle lanes stay in bounds and in the ballots
    const int64_t o0 = ch * chunk, o1 = min(o0 + chunk, nout);
    const int64_t col = col0 + (p / nbins) * nb + p % nbins;
    const int64_t at = y * g.nx + x;
    const uint16_t *in = ys + p * g.nvox + at;
    uint32_t s = 0;
    for (int64_t z = o0; z < o0 + g.sz - 1; ++z) s += in[z * plane];
    for (int64_t o = o0; o < o1; ++o) {
      s += in[(o + g.sz - 1) * plane];
      const int64_t zc = o + g.hz;
      const bool on = live && flag[zc * plane + at] != 0;
      const uint64_t m = __builtin_amdgcn_ballot_w64(on);
      if (on) {
        const int64_t number = (int64_t)seg_base[seg + g.gx * (y + g.ny * zc)] + lanes_below(m) - row0;
        counts[number * row_stride + col * col_stride] = s;
      }
      s -= in[o * plane];
    }
  }
}

// first[o] = number of the first region of centre plane hz + o (seg_base of the plane's first
// segment), for the block plan on the host.
__global__ __launch_bounds__(256) void dense_plane_first_kernel(const uint32_t *__restrict__ seg_base,
                                                                uint32_t *__restrict__ first, int64_t plane_segs,
                                                                int64_t hz, int64_t nplanes) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o < nplanes) first[o] = seg_base[(hz + o) * plane_segs];
}

// The planar block planar[column][row in block] (ld words per column) to the row-major block
// rows[row in block][nhist][nb] that goes to the host.  FREQ: every histogram as
// DenseHistogram::getFrequencies forms it (DenseHistogram.h:55-60): the nb counts summed into an
// int, then (float)count / (float)sum, NaN throughout for an empty histogram; else the counts.
//
// A workgroup stages a tile of 2^tr_log2 rows x `hists` whole histograms in LDS, a column of the
// tile at pitch rows + 1 words.  In: lanes along the rows of one column, contiguous in global
// memory and in LDS.  Sums: a thread per (row, histogram), lanes along rows, LDS addresses
// consecutive; the quotients replace the counts in place.  Out: lanes along the words of an output
// row (and on into the next row of the tile: one run when the tile spans the row), LDS addresses
// pitch words apart -- the pitch is odd, so the 32 lanes of a half wave fall on 32 different banks.
// Nothing is assumed to divide: the last tile of rows and the last group of histograms are partial.
// Grid: x = row tiles, y = histogram groups (strided when there are more than the grid holds).
constexpr int DENSE_FREQ_LDS_WORDS = 12288;  // 48 KiB
template <bool FREQ>
__global__ __launch_bounds__(256) void dense_freq_kernel(const uint32_t *__restrict__ planar,
                                                         uint32_t *__restrict__ rows, int64_t n_rows,
                                                         int64_t ld, int nhist, int nb, int hists,
                                                         int tr_log2) {
  __shared__ uint32_t tile[DENSE_FREQ_LDS_WORDS];
  const int tr = 1 << tr_log2, pitch = tr + 1;
  const int64_t r0 = (int64_t)blockIdx.x * tr, row_words = (int64_t)nhist * nb;
  const int nr = (int)min((int64_t)tr, n_rows - r0);
  for (int h0 = blockIdx.y * hists; h0 < nhist; h0 += gridDim.y * hists) {
    const int nh = min(hists, nhist - h0), wt = nh * nb;
    const int64_t w0 = (int64_t)h0 * nb;
    for (int i = threadIdx.x; i < wt << tr_log2; i += blockDim.x) {
      const int c = i >> tr_log2, r = i & (tr - 1);
      if (r < nr) tile[c * pitch + r] = planar[(w0 + c) * ld + r0 + r];
    }
    __syncthreads();
    if (FREQ) {
      for (int i = threadIdx.x; i < nh << tr_log2; i += blockDim.x) {
        const int h = i >> tr_log2, r = i & (tr - 1);
        if (r < nr) {
          uint32_t *t = tile + h * nb * pitch + r;
          uint32_t sum = 0;
          for (int b = 0; b < nb; ++b) sum += t[b * pitch];
          const float d = (float)(int)sum;
          for (int b = 0; b < nb; ++b) t[b * pitch] = __float_as_uint((float)t[b * pitch] / d);
        }
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < nr * wt; i += blockDim.x) {
      const int r = i / wt, j = i - r * wt;
      rows[(r0 + r) * row_words + w0 + j] = tile[j * pitch + r];
    }
    __syncthreads();
  }
}

}  // namespace ife
#endif
