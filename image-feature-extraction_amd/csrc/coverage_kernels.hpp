// coverage_kernels.hpp -- the kernels of ife_value_census_f32, ife_threshold_mask and
// ife_roi_coverage (include/ife_hip.h, DESIGN.md "Census and coverage").  Integer only: floats are
// read as bits and decided by coverage_plan.hpp's integer images.
//
//   census    over the sorted copy (negative NaNs first, positive NaNs last, -0 next to +0):
//     heads      a wave per segment of CENSUS_SEG elements: the ballot of "no NaN, and the first
//                element or another value than its predecessor", its popcount per segment; the
//                NaNs of either sign counted on the way
//     (scan)     chunk_sum / scan_chunks / chunk_scan of stats_kernels.hpp: run heads before
//                every segment, the number of runs in front
//     positions  the same ballots once more: head number r writes its position
//     runs       run r: its value (-0 as +0) and the distance to the next head; the last run
//                ends where the positive NaNs begin
//   threshold 16-byte pieces of the image from its first aligned element, four mask bytes per
//             lane in one store where the mask is aligned there, the ends one by one
//   coverage  two planes of one bit per voxel, bit (i & 31) of word (i >> 5) for voxel i:
//     plane      a wave per 256 voxels, four ballots of `mask != 0`, eight words; their
//                popcounts are region_size
//     paint      a wave per box, a lane per box row: the row's bit range (coverage_plan.hpp) is
//                OR-ed into the visited plane word by word
//     count      popc(visited) and popc(visited & mask) over the words
#ifndef IFE_COVERAGE_KERNELS_HPP
#define IFE_COVERAGE_KERNELS_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coverage_plan.hpp"
#include "stats_kernels.hpp"

namespace ife {

constexpr int CENSUS_SEG = 256;                  // sorted elements per wave and segment count
constexpr int64_t CENSUS_GRID_CAP = 1024;        // workgroups of the two segment walks, four segments each
constexpr int64_t THRESHOLD_GRID_CAP = 2048;     // one add to the counter per workgroup
constexpr int COVERAGE_GROUP = 256;              // voxels per wave and trip of the plane kernel
constexpr int64_t COVERAGE_PLANE_GRID_CAP = 2048;
constexpr int64_t COVERAGE_PAINT_GRID_CAP = 1024;  // workgroups of four boxes each
constexpr int64_t COVERAGE_COUNT_GRID_CAP = 1024;

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The sum over a workgroup of 256 threads, valid in thread 0; tmp holds 4 words.  The counters of
// these kernels are single words: one add per workgroup, since adds to one address go one by one.
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t *tmp) {
  v = wave_sum_u32(v);
  if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  v = tmp[0] + tmp[1] + tmp[2] + tmp[3];
  __syncthreads();
  return v;
}

// ---- census ------------------------------------------------------------------------------------------
// nans[0]: negative NaNs, nans[1]: positive NaNs (zeroed by the caller)
__device__ __forceinline__ bool census_head(const uint32_t *__restrict__ s, int64_t i, int64_t n, bool *nan) {
  *nan = false;
  if (i >= n) return false;
  const uint32_t u = s[i];
  if (coverage_is_nan(u)) { *nan = true; return false; }
  if (i == 0) return true;
  const uint32_t p = s[i - 1];
  return coverage_is_nan(p) || census_canonical(p) != census_canonical(u);
}

__global__ __launch_bounds__(256) void census_heads_kernel(const uint32_t *__restrict__ sorted, int64_t n,
                                                           int64_t nseg, uint32_t *__restrict__ seg_heads,
                                                           unsigned long long *__restrict__ nans) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  uint32_t neg = 0, pos = 0;
  for (int64_t seg = wave0; seg < nseg; seg += nwaves) {
    uint32_t heads = 0;
#pragma unroll
    for (int r = 0; r < CENSUS_SEG / 64; ++r) {
      const int64_t i = seg * CENSUS_SEG + r * 64 + lane;
      bool nan;
      const bool head = census_head(sorted, i, n, &nan);
      heads += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(head));
      const bool negative = nan && (sorted[i] >> 31);
      neg += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(negative));
      pos += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(nan && !negative));
    }
    if (lane == 0) seg_heads[seg] = heads;
  }
  if (lane == 0) {
    if (neg) atomicAdd(&nans[0], (unsigned long long)neg);
    if (pos) atomicAdd(&nans[1], (unsigned long long)pos);
  }
}

// bases: seg_heads after the scan.  positions[r] = the index of head r in the sorted copy.
__global__ __launch_bounds__(256) void census_positions_kernel(const uint32_t *__restrict__ sorted, int64_t n,
                                                               int64_t nseg, const uint32_t *__restrict__ bases,
                                                               uint32_t *__restrict__ positions) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t seg = wave0; seg < nseg; seg += nwaves) {
    uint32_t run = bases[seg];
#pragma unroll
    for (int r = 0; r < CENSUS_SEG / 64; ++r) {
      const int64_t i = seg * CENSUS_SEG + r * 64 + lane;
      bool nan;
      const bool head = census_head(sorted, i, n, &nan);
      const uint64_t m = __builtin_amdgcn_ballot_w64(head);
      if (head) positions[run + lanes_below(m)] = (uint32_t)i;
      run += (uint32_t)__popcll(m);
    }
  }
}

// end: where the positive NaNs begin
__global__ __launch_bounds__(256) void census_runs_kernel(const uint32_t *__restrict__ sorted,
                                                          const uint32_t *__restrict__ positions,
                                                          int64_t n_unique, uint32_t end,
                                                          uint32_t *__restrict__ uniq, uint32_t *__restrict__ counts) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_unique;
       r += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t p = positions[r];
    const uint32_t next = r + 1 < n_unique ? positions[r + 1] : end;
    uniq[r] = census_canonical(sorted[p]);
    counts[r] = next - p;
  }
}

// ---- threshold ---------------------------------------------------------------------------------------
// head: the elements in front of the first 16-byte aligned one (at most 3, at most n); packed: the
// mask is 4-byte aligned at element `head`.  *count (zeroed by the caller) receives the ones.
__global__ __launch_bounds__(256) void threshold_mask_kernel(const uint32_t *__restrict__ image, int64_t n,
                                                             int64_t head, int32_t low, int32_t high, bool packed,
                                                             uint8_t *__restrict__ mask,
                                                             unsigned long long *__restrict__ count) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t npieces = (n - head) >> 2, tail0 = head + 4 * npieces;
  uint32_t ones = 0;
  const uint4 *pieces = reinterpret_cast<const uint4 *>(image + head);
  for (int64_t k = tid; k < npieces; k += nthreads) {
    const uint4 v = pieces[k];
    const uint32_t b0 = threshold_inside(v.x, low, high), b1 = threshold_inside(v.y, low, high),
                   b2 = threshold_inside(v.z, low, high), b3 = threshold_inside(v.w, low, high);
    uint8_t *m = mask + head + 4 * k;
    if (packed) {
      *reinterpret_cast<uint32_t *>(m) = b0 | b1 << 8 | b2 << 16 | b3 << 24;
    } else {
      m[0] = (uint8_t)b0; m[1] = (uint8_t)b1; m[2] = (uint8_t)b2; m[3] = (uint8_t)b3;
    }
    ones += b0 + b1 + b2 + b3;
  }
  // the ends, each shorter than a piece: three threads each
  if (tid < 6) {
    const int64_t e = tid < 3 ? tid : tail0 + (tid - 3);
    if (tid < 3 ? e < head : e < n) {
      const uint32_t b = threshold_inside(image[e], low, high);
      mask[e] = (uint8_t)b;
      ones += b;
    }
  }
  __shared__ uint32_t tmp[4];
  ones = block_sum_u32(ones, tmp);  // below 2^32: a workgroup takes at most 2^40 / 2048 elements
  if (threadIdx.x == 0 && ones) atomicAdd(count, (unsigned long long)ones);
}

// ---- coverage ----------------------------------------------------------------------------------------
struct CoverageCounters {
  unsigned long long region;
  unsigned long long visited[COVERAGE_MAX_ROUNDS], hits[COVERAGE_MAX_ROUNDS];
  int bad;
};

// plane: ceil(nvox / 256) * 8 words, all of them written; bits at and beyond nvox are 0
template <typename TM>
__global__ __launch_bounds__(256) void coverage_plane_kernel(const TM *__restrict__ mask, int64_t nvox,
                                                             uint32_t *__restrict__ plane,
                                                             CoverageCounters *__restrict__ c) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t ngroups = (nvox + COVERAGE_GROUP - 1) / COVERAGE_GROUP;
  uint32_t ones = 0;
  for (int64_t g = wave0; g < ngroups; g += nwaves) {
    bool on[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // the four loads are issued before the first ballot waits
      const int64_t i = g * COVERAGE_GROUP + r * 64 + lane;
      on[r] = i < nvox && mask[i] != 0;
    }
    uint64_t mine = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint64_t m = __builtin_amdgcn_ballot_w64(on[r]);
      ones += (uint32_t)__popcll(m);
      if (lane == r) mine = m;
    }
    if (lane < 4) reinterpret_cast<unsigned long long *>(plane)[g * 4 + lane] = mine;  // little endian: word 2k first
  }
  __shared__ uint32_t tmp[4];
  if (lane != 0) ones = 0;  // every lane holds the wave's count
  ones = block_sum_u32(ones, tmp);
  if (threadIdx.x == 0 && ones) atomicAdd(&c->region, (unsigned long long)ones);
}

// DEVICE boxes cannot be checked on the host: c->bad = 1 where one has a size below 1 or leaves the volume
__global__ __launch_bounds__(256) void coverage_box_check_kernel(const int64_t *__restrict__ rois, int64_t n_rois,
                                                                 int64_t nx, int64_t ny, int64_t nz,
                                                                 CoverageCounters *__restrict__ c) {
  const int64_t n[3] = {nx, ny, nz};
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rois; r += (int64_t)gridDim.x * blockDim.x)
    if (!coverage_box_ok(rois + 6 * r, n)) c->bad = 1;
}

// boxes [k0, k1), all inside the volume (checked): a wave per box, a lane per row of it
__global__ __launch_bounds__(256) void coverage_paint_kernel(const int64_t *__restrict__ rois, int64_t k0,
                                                             int64_t k1, int64_t nx, int64_t ny,
                                                             uint32_t *__restrict__ visited) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t k = k0 + wave0; k < k1; k += nwaves) {
    const int64_t *q = rois + 6 * k;
    const int64_t x0 = q[0], y0 = q[1], z0 = q[2], sx = q[3], sy = q[4], sz = q[5];
    const int64_t nrows = sy * sz;
    for (int64_t row = lane; row < nrows; row += 64) {
      const int64_t zz = row / sy, yy = row - zz * sy;
      const CoverageBits b = coverage_bit_range(((z0 + zz) * ny + (y0 + yy)) * nx + x0, sx);
      for (int64_t w = b.w0; w <= b.w1; ++w) atomicOr(&visited[w], coverage_word_bits(b, w));
    }
  }
}

// c->visited[round] += popc(visited), c->hits[round] += popc(visited & mask) over nwords words; tail: the
// voxel bits of the last word
__global__ __launch_bounds__(256) void coverage_count_kernel(const uint32_t *__restrict__ visited,
                                                             const uint32_t *__restrict__ plane, int64_t nwords,
                                                             uint32_t tail, int round,
                                                             CoverageCounters *__restrict__ c) {
  uint32_t nv = 0, nh = 0;  // a workgroup sees at most 2^32 voxels
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (int64_t)gridDim.x * blockDim.x) {
    uint32_t v = visited[w];
    if (w == nwords - 1) v &= tail;
    nv += (uint32_t)__popc(v);
    nh += (uint32_t)__popc(v & plane[w]);
  }
  __shared__ uint32_t tmp[4];
  nv = block_sum_u32(nv, tmp);
  nh = block_sum_u32(nh, tmp);
  if (threadIdx.x == 0) {
    if (nv) atomicAdd(&c->visited[round], (unsigned long long)nv);
    if (nh) atomicAdd(&c->hits[round], (unsigned long long)nh);
  }
}

}  // namespace ife

#endif  // IFE_COVERAGE_KERNELS_HPP
