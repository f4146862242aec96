// labels_kernels.hpp -- device side of the per-region label modes (tools/ExtractLabels.cxx): the
// label of a region is the mode of a uint8 label volume inside its box, under a set G of ignored
// labels and an optional dominant label d.  The rule (include/ife_hip.h): with
// n(l) the number of voxels of the box that carry l and c(l) = 0 for l in G, else n(l),
//   1. d >= 0 and (n(d) > 0 or d in G): d
//   2. else max c > 0: the smallest l with c(l) = max c
//   3. else: the smallest member of G
//
// Box list (roi_labels_kernel): a workgroup per box, 256 counters in LDS.  Label maps are
// piecewise constant, so a wave counts by its distinct values (wave_distinct): one LDS add per
// value and wave instead of 64 adds on one address.  The rule is a reduction over the counters;
// every out byte has one writer and nothing is added in global memory.
//
// Dense (one region per centre of dense_kernels.hpp, all boxes of one size): n(l) at every centre
// is the 3-D box sum of the indicator "the voxel carries l", so the centres, the x pass and the y
// pass of dense_kernels.hpp are taken as they are with the label in the place of the bin code:
//   presence  which of the 256 values occur in the volume; only those get planes
//   codes     per group of at most 255 labels one byte per voxel: the label's place in the group,
//             DENSE_OUTSIDE for a label of another group (so all 256 values are served)
//   x, y      dense_box_x_kernel, dense_box_y_kernel
//   z, mode   label_mode_z_kernel, one launch per label in a fixed order: the running sum along z
//             is n(l) at the centre; it replaces the region's (best count, label) pair where it is
//             strictly greater.  Labels go through in ascending order, ignored ones not at all,
//             and the dominant label last in a form that takes the region wherever n(d) > 0.
// The pair is 5 bytes per region (the label byte is the output itself, preset to the answer of
// clause 3), has one writer per launch, and the launches are ordered by the stream.
#ifndef IFE_LABELS_KERNELS_HPP
#define IFE_LABELS_KERNELS_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_kernels.hpp"

namespace ife {

constexpr int LABEL_VALUES = 256;
constexpr int LABELS_GRID_CAP = 1 << 14;  // workgroups of roi_labels_kernel; beyond, a workgroup takes several boxes
constexpr int64_t LABELS_MAX_BOX = 0xffffffffll;  // voxels per box: the counters are 32 bits wide

struct LabelRule {
  uint32_t ignore[8];  // bit l of word l / 32: l is in G
  int dominant;        // -1: none
  int fallback;        // clause 3: the smallest member of G (0 where G is empty: never taken)
};

__device__ __forceinline__ bool label_ignored(const LabelRule &r, int l) { return (r.ignore[l >> 5] >> (l & 31)) & 1u; }

// The distinct values among the active lanes of a wave: f(value, number of lanes that hold it),
// called in the lane that holds the value first.  Every lane of the wave must call this.
template <typename F>
__device__ __forceinline__ void wave_distinct(int value, bool active, F &&f) {
  const int lane = threadIdx.x & 63;
  uint64_t left = __builtin_amdgcn_ballot_w64(active);
  while (left) {
    const int first = __ffsll((unsigned long long)left) - 1;
    const int v = __shfl(value, first, 64);
    const uint64_t same = __builtin_amdgcn_ballot_w64(active && value == v);
    if (lane == first) f(v, (uint32_t)__popcll(same));
    left &= ~same;
  }
}

__device__ __forceinline__ bool label_box_ok(const int64_t *q, int64_t nx, int64_t ny, int64_t nz) {
  // sizes first: with 1 <= size <= n the volume below cannot overflow
  if (q[3] < 1 || q[4] < 1 || q[5] < 1 || q[3] > nx || q[4] > ny || q[5] > nz) return false;
  if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[0] > nx - q[3] || q[1] > ny - q[4] || q[2] > nz - q[5]) return false;
  return q[3] * q[4] <= LABELS_MAX_BOX / q[5];
}

// DEVICE mode: the boxes cannot be checked on the host.  *bad = 1 where a box leaves the volume,
// has a size below 1 or more voxels than the counters hold (the host zeroes it first; every
// writer stores the same value).
__global__ __launch_bounds__(256) void roi_check_kernel(const int64_t *__restrict__ rois, int64_t n_rois,
                                                        int64_t nx, int64_t ny, int64_t nz,
                                                        int *__restrict__ bad) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rois; r += (int64_t)gridDim.x * blockDim.x)
    if (!label_box_ok(rois + 6 * r, nx, ny, nz)) *bad = 1;
}

// out[r] = the label of box r.  Grid: min(n_rois, LABELS_GRID_CAP) workgroups of 256.
__global__ __launch_bounds__(256) void roi_labels_kernel(const uint8_t *__restrict__ labels,
                                                         const int64_t *__restrict__ rois, int64_t n_rois,
                                                         int64_t nx, int64_t ny, LabelRule rule,
                                                         uint8_t *__restrict__ out) {
  __shared__ uint32_t c[LABEL_VALUES];
  __shared__ unsigned long long top[4];
  const int tid = threadIdx.x;
  for (int64_t r = blockIdx.x; r < n_rois; r += gridDim.x) {
    c[tid] = 0;
    __syncthreads();
    const int64_t *q = rois + 6 * r;
    const int64_t x0 = q[0], y0 = q[1], z0 = q[2], sx = q[3], sy = q[4], sz = q[5];
    const int64_t n = sx * sy * sz;
    for (int64_t t0 = 0; t0 < n; t0 += 256) {  // the same trip count in every lane: the ballots need whole waves
      const int64_t t = t0 + tid;
      const bool active = t < n;
      int v = 0;
      if (active) {
        const int64_t x = t % sx, y = (t / sx) % sy, z = t / (sx * sy);
        v = labels[(x0 + x) + nx * ((y0 + y) + ny * (z0 + z))];
      }
      wave_distinct(v, active, [&](int value, uint32_t count) { atomicAdd(&c[value], count); });
    }
    __syncthreads();
    // the largest count that is not ignored, the smallest label among equals: the maximum of
    // count * 256 + (255 - label)
    const uint32_t mine = label_ignored(rule, tid) ? 0u : c[tid];
    const uint32_t n_dominant = rule.dominant >= 0 ? c[rule.dominant] : 0u;
    unsigned long long key = ((unsigned long long)mine << 8) | (unsigned)(255 - tid);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o, 64);
      key = other > key ? other : key;
    }
    if ((tid & 63) == 0) top[tid >> 6] = key;
    __syncthreads();  // every lane has read its counters: the next box may zero them
    if (tid == 0) {
      for (int w = 1; w < 4; ++w) key = top[w] > key ? top[w] : key;
      int label = rule.fallback;
      if (rule.dominant >= 0 && (n_dominant > 0 || label_ignored(rule, rule.dominant))) label = rule.dominant;
      else if (key >> 8) label = 255 - (int)(key & 255);
      out[r] = (uint8_t)label;
    }
  }
}

// present[l] = 1 where some voxel carries l (the host zeroes present[256] first; every writer
// stores the same value).
__global__ __launch_bounds__(256) void label_presence_kernel(const uint8_t *__restrict__ labels, int64_t nvox,
                                                             uint32_t *__restrict__ present) {
  __shared__ uint32_t seen[LABEL_VALUES];
  seen[threadIdx.x] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < nvox; i0 += stride) {
    const int64_t i = i0 + threadIdx.x;
    const bool active = i < nvox;
    const int v = active ? labels[i] : 0;
    wave_distinct(v, active, [&](int value, uint32_t) { seen[value] = 1; });
  }
  __syncthreads();
  if (seen[threadIdx.x]) present[threadIdx.x] = 1;
}

// code[i] = lut[labels[i]]: the place of the voxel's label in the group, DENSE_OUTSIDE otherwise.
__global__ __launch_bounds__(256) void label_code_kernel(const uint8_t *__restrict__ labels,
                                                         const uint8_t *__restrict__ lut,
                                                         uint8_t *__restrict__ code, int64_t nvox) {
  __shared__ uint8_t l[LABEL_VALUES];
  l[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x)
    code[i] = l[labels[i]];
}

// z pass of ONE label's plane in the mode form: the running sum of ys along z is n(label) in the
// box around (x, y, z).  At a centre it replaces the region's pair (best[number], out[number])
// where it is strictly greater than best; `force` (the dominant label): wherever it is positive.
// Lanes along x, a wave marches `chunk` planes of one (segment, y); a region lies in exactly one
// of them.  nwork = gx * (ny - sy + 1) * nchunks.
__global__ __launch_bounds__(256) void label_mode_z_kernel(const uint16_t *__restrict__ ys,
                                                           const uint8_t *__restrict__ flag,
                                                           const uint32_t *__restrict__ seg_base,
                                                           uint32_t *__restrict__ best, uint8_t *__restrict__ out,
                                                           DenseGeom g, int label, int force, int chunk,
                                                           int nchunks, int64_t nwork) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t nyv = g.ny - g.sy + 1, nout = g.nz - g.sz + 1, plane = g.nx * g.ny;
  for (int64_t w = wave0; w < nwork; w += nwaves) {
    int64_t t = w;
    const int64_t seg = t % g.gx; t /= g.gx;
    const int64_t y = t % nyv + g.hy, ch = t / nyv;
    const bool live = seg * 64 + lane < g.nx;
    const int64_t x = live ? seg * 64 + lane : g.nx - 1;  // idle lanes stay in bounds and in the ballots
    const int64_t o0 = ch * chunk, o1 = min(o0 + chunk, nout);
    const int64_t at = y * g.nx + x;
    const uint16_t *in = ys + at;
    uint32_t s = 0;
    for (int64_t z = o0; z < o0 + g.sz - 1; ++z) s += in[z * plane];
    for (int64_t o = o0; o < o1; ++o) {
      s += in[(o + g.sz - 1) * plane];
      const int64_t zc = o + g.hz;
      const bool on = live && flag[zc * plane + at] != 0;
      const uint64_t m = __builtin_amdgcn_ballot_w64(on);
      if (on) {
        const int64_t number = (int64_t)seg_base[seg + g.gx * (y + g.ny * zc)] + lanes_below(m);
        if (force ? s > 0 : s > best[number]) {
          best[number] = s;
          out[number] = (uint8_t)label;
        }
      }
      s -= in[o * plane];
    }
  }
}

}  // namespace ife
#endif
