// sampling_kernels.hpp -- the kernels of ife_sample_positions, ife_random_rois and
// ife_extract_rois (include/ife_hip.h, DESIGN.md "Sampling").  Integer only.
//
//   count   a wave per 64-voxel row segment, lanes along x (dense_centre_kernel's layout), a run of
//           consecutive segments per wave: per value set the ballot of "in the set and the box
//           fits", its popcount into counts[set][segment]; all sets from one read of the mask, no
//           flag per voxel
//   scan    chunk_sum / scan_chunks / chunk_scan of stats_kernels.hpp, per set: the counts become
//           the number of admissible voxels before every segment, the total stands in front
//   select  one wave per draw: the rank from the generator (sampling_plan.hpp), the last segment
//           whose base is <= rank (empty segments share the base of their successor, so the last
//           one is the one that holds the voxel), the segment's ballot once more from the mask;
//           the lane with `rank - base` admissible lanes below it writes
//   gather  one wave per row of a box: aligned 16-byte pieces of the output row from any byte
//           offset of the source (region_kernels.hpp), the ends short of a piece one by one
#ifndef IFE_SAMPLING_KERNELS_HPP
#define IFE_SAMPLING_KERNELS_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_kernels.hpp"
#include "region_kernels.hpp"
#include "sampling_plan.hpp"

namespace ife {

constexpr int64_t SAMPLING_COUNT_RUN = 8;  // consecutive row segments per wave of the count pass
constexpr int64_t SAMPLING_SELECT_GRID_CAP = 1 << 16;
constexpr int64_t SAMPLING_GATHER_GRID_CAP = 4096;

// counts: set j's segment counts at counts + j * set_stride (words).
template <typename TM>
__global__ __launch_bounds__(256) void sampling_count_kernel(const TM *__restrict__ mask,
                                                             uint32_t *__restrict__ counts, int64_t set_stride,
                                                             DenseGeom g, int64_t nseg, SamplingSets sets) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // a wave takes a run of consecutive segments: the divisions that place a segment are paid once
  // per run, after that the position is carried
  const int64_t per = (nseg + nwaves - 1) / nwaves;
  const int64_t s0 = wave * per, s1 = min(nseg, s0 + per);
  if (s0 >= s1) return;
  int64_t row = s0 / g.gx, bx = s0 - row * g.gx;
  int64_t z = row / g.ny, y = row - z * g.ny;
  // four segments at a time: their loads are issued before the first ballot waits for one
  for (int64_t s = s0; s < s1; s += 4) {
    bool fits[4];
    uint32_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t x = bx * 64 + lane;
      fits[u] = s + u < s1 && x < g.nx && dense_fits(g, x, y, z);
      v[u] = fits[u] ? (uint32_t)mask[row * g.nx + x] : 0u;
      if (++bx == g.gx) {
        bx = 0;
        ++row;
        if (++y == g.ny) { y = 0; ++z; }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (s + u >= s1) break;  // wave-uniform
      for (int j = 0; j < sets.n_sets; ++j) {
        const uint64_t m = __builtin_amdgcn_ballot_w64(fits[u] && sampling_member(sets, j, v[u]));
        if (lane == 0) counts[j * set_stride + s + u] = (uint32_t)__popcll(m);
      }
    }
  }
}

struct SamplingDraws {
  uint64_t seed, first_draw;
  uint32_t stream;
  int64_t n_draws;
  int boxes;  // 0: out[set][draw] = linear index; 1: out[set][draw][6] = the box around the voxel
};

// bases: set j's scanned counts at bases + j * set_stride (words), its total (64 bits) two words
// in front of them.  Wave w takes draw w % n_draws of set w / n_draws.
template <typename TM>
__global__ __launch_bounds__(256) void sampling_select_kernel(const TM *__restrict__ mask,
                                                              const uint32_t *__restrict__ bases, int64_t set_stride,
                                                              DenseGeom g, int64_t nseg, SamplingSets sets,
                                                              SamplingDraws d, int64_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t total = d.n_draws * sets.n_sets;
  for (int64_t w = wave0; w < total; w += nwaves) {
    const int j = (int)(w / d.n_draws);
    const uint64_t k = d.first_draw + (uint64_t)(w % d.n_draws);
    const uint32_t *b = bases + j * set_stride;
    const uint64_t n = *reinterpret_cast<const unsigned long long *>(b - 2);
    if (n == 0) continue;  // the host does not launch for an empty set
    const uint32_t r = (uint32_t)sampling_rank(d.seed, d.stream + (uint32_t)j, k, n);  // below n < 2^32
    int64_t lo = 0, hi = nseg;  // b[0] == 0 <= r: the answer is lo - 1 >= 0
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (b[mid] <= r) lo = mid + 1; else hi = mid;
    }
    const int64_t s = lo - 1;
    const uint32_t rem = r - b[s];
    const int64_t row = s / g.gx;
    const int64_t x = (s % g.gx) * 64 + lane;
    const int64_t y = row % g.ny, z = row / g.ny;
    const bool on = x < g.nx && dense_fits(g, x, y, z) && sampling_member(sets, j, (uint32_t)mask[row * g.nx + x]);
    const uint64_t m = __builtin_amdgcn_ballot_w64(on);
    if (on && lanes_below(m) == rem) {
      if (d.boxes) {
        int64_t *q = out + 6 * w;
        q[0] = x - g.hx; q[1] = y - g.hy; q[2] = z - g.hz;
        q[3] = g.sx; q[4] = g.sy; q[5] = g.sz;
      } else {
        out[w] = row * g.nx + x;
      }
    }
  }
}

// DEVICE mode: the boxes cannot be checked on the host.  *bad = 1 where a box has not the size
// {sx, sy, sz} (of the first box, read back and checked by the host) or leaves the volume.
__global__ __launch_bounds__(256) void sampling_box_check_kernel(const int64_t *__restrict__ rois, int64_t n_rois,
                                                                 int64_t sx, int64_t sy, int64_t sz, int64_t nx,
                                                                 int64_t ny, int64_t nz, int *__restrict__ bad) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rois; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t *q = rois + 6 * r;
    if (q[3] != sx || q[4] != sy || q[5] != sz || q[0] < 0 || q[1] < 0 || q[2] < 0 || q[0] > nx - sx ||
        q[1] > ny - sy || q[2] > nz - sz)
      *bad = 1;
  }
}

// dst[box][z][y][x] = src[box.z0 + z][box.y0 + y][box.x0 + x], ES bytes per element.  nrows =
// n_rois * sy * sz; every box has the size {sx, sy, sz} and lies inside the volume (checked).
template <int ES>
__global__ __launch_bounds__(REGION_BLOCK) void sampling_gather_kernel(const unsigned char *__restrict__ src,
                                                                        const int64_t *__restrict__ rois,
                                                                        int64_t nrows, int64_t sx, int64_t sy,
                                                                        int64_t sz, int64_t nx, int64_t ny,
                                                                        unsigned char *__restrict__ dst) {
  typedef typename RegionElem<ES>::type T;
  constexpr int64_t EPP = 16 / ES;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * REGION_WAVES;
  for (int64_t r = (int64_t)blockIdx.x * REGION_WAVES + (threadIdx.x >> 6); r < nrows; r += stride) {
    const int64_t box = r / (sy * sz), in_box = r - box * (sy * sz);
    const int64_t zz = in_box / sy, yy = in_box - zz * sy;
    const int64_t *q = rois + 6 * box;
    const unsigned char *srow = src + (size_t)(((q[2] + zz) * ny + (q[1] + yy)) * nx + q[0]) * ES;
    unsigned char *drow = dst + (size_t)r * (size_t)sx * ES;
    const int64_t head = min(sx, (int64_t)((0 - reinterpret_cast<uintptr_t>(drow)) & 15u) / ES);
    const int64_t nb = (sx - head) / EPP, tail0 = head + nb * EPP;
    uint4 *dpieces = reinterpret_cast<uint4 *>(drow + (size_t)head * ES);
    for (int64_t k = lane; k < nb; k += 64) dpieces[k] = region_load16(srow + (size_t)(head + k * EPP) * ES);
    // head and tail, each shorter than a piece: 16 lanes each
    if (lane < 32) {
      const bool at_tail = lane >= 16;
      const int64_t e = at_tail ? tail0 + (lane - 16) : lane;
      if (e < (at_tail ? sx : head)) reinterpret_cast<T *>(drow)[e] = reinterpret_cast<const T *>(srow)[e];
    }
  }
}

}  // namespace ife

#endif  // IFE_SAMPLING_KERNELS_HPP
