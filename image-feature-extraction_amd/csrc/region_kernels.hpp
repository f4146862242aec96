// region_kernels.hpp -- the kernels of ife_mask_bounding_box, ife_extract_region and
// ife_label_membership (include/ife_hip.h, DESIGN.md "Regions").  All three pass once over their
// data and are bound by memory: the steady parts move 16-byte pieces, the ends of a run that do
// not fill an aligned piece go element by element, and the grids are min(work, cap) workgroups
// that loop.
#ifndef IFE_REGION_KERNELS_HPP
#define IFE_REGION_KERNELS_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "region_plan.hpp"

constexpr int REGION_BLOCK = 256;
constexpr int REGION_WAVES = REGION_BLOCK / 64;
// bounding box: a workgroup takes a unit of whole rows of about this many bytes (one row where a
// row is longer), at most REGION_BOX_GRID_CAP workgroups
constexpr int64_t REGION_BOX_UNIT_BYTES = 16384;
constexpr int64_t REGION_BOX_GRID_CAP = 2048;
// extract: a wave takes an output row, a workgroup REGION_WAVES of them
constexpr int64_t REGION_EXTRACT_GRID_CAP = 4096;
constexpr int64_t REGION_MEMBER_GRID_CAP = 2048;

// what the box kernel leaves: the corners as unsigned (min preset to all ones, max to zero) and
// the number of foreground voxels
struct RegionBoxRecord {
  uint32_t lo[3];
  uint32_t hi[3];
  unsigned long long count;
};
static_assert(sizeof(RegionBoxRecord) == 32, "six words and a 64-bit count");

// 16 bytes from any byte address (the hardware takes unaligned global accesses)
struct __attribute__((packed, aligned(1))) RegionPiece {
  uint32_t w[4];
};
__device__ inline uint4 region_load16(const unsigned char *p) {
  const RegionPiece v = *reinterpret_cast<const RegionPiece *>(p);
  return make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
}

// ---- bounding box ----------------------------------------------------------------------------
// bit i set: element i of the piece is foreground.  FLOATBITS: anything but +-0.
template <int ES, bool FLOATBITS>
__device__ inline uint32_t region_nonzero_bits(const uint4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
  if (ES == 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) m |= ((w[i >> 2] >> (8 * (i & 3))) & 0xffu) ? (1u << i) : 0u;
  } else if (ES == 2) {
#pragma unroll
    for (int i = 0; i < 8; ++i) m |= ((w[i >> 1] >> (16 * (i & 1))) & 0xffffu) ? (1u << i) : 0u;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) m |= (FLOATBITS ? (w[i] & 0x7fffffffu) : w[i]) ? (1u << i) : 0u;
  }
  return m;
}

struct RegionBoxAcc {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
  uint32_t hi[3] = {0u, 0u, 0u};
  unsigned long long count = 0;
  __device__ void add(uint32_t x, uint32_t y, uint32_t z) {
    lo[0] = min(lo[0], x); hi[0] = max(hi[0], x);
    lo[1] = min(lo[1], y); hi[1] = max(hi[1], y);
    lo[2] = min(lo[2], z); hi[2] = max(hi[2], z);
  }
};

// mask: nrows rows of nx elements of ES bytes (rows = ny * nz, dense).  Unit u holds the rows
// [u * rows_per_unit, ...): a contiguous run whose aligned 16-byte pieces are read whole and whose
// first and last elements, short of a piece, one by one.  A piece of zeros costs its load and one
// compare.
template <int ES, bool FLOATBITS>
__global__ __launch_bounds__(REGION_BLOCK) void region_box_kernel(const unsigned char *__restrict__ mask, uint32_t nx,
                                                                   uint32_t ny, int64_t nrows, int64_t rows_per_unit,
                                                                   int64_t nunits, RegionBoxRecord *rec) {
  constexpr uint32_t EPP = 16 / ES;
  RegionBoxAcc acc;
  for (int64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int64_t r0 = u * rows_per_unit;
    const int64_t nr = min(rows_per_unit, nrows - r0);
    // rows_per_unit > 1 only where a unit is at most REGION_BOX_UNIT_BYTES: 32 bits hold nelem
    const uint32_t nelem = (uint32_t)nr * nx;
    const unsigned char *base = mask + (size_t)r0 * nx * ES;
    const uint32_t y0 = (uint32_t)(r0 % ny);
    const int64_t z0 = r0 / ny;
    const uint32_t head = min(nelem, (uint32_t)((0 - reinterpret_cast<uintptr_t>(base)) & 15u) / ES);
    const uint32_t npieces = (nelem - head) / EPP;
    const uint32_t tail0 = head + npieces * EPP;
    // element e of the unit -> (x, y, z)
    auto locate = [&](uint32_t e, uint32_t &x, uint32_t &y, uint32_t &z) {
      const uint32_t row = e / nx;
      x = e - row * nx;
      const uint32_t yy = y0 + row;  // below ny + 16384
      const uint32_t dz = yy / ny;
      y = yy - dz * ny;
      z = (uint32_t)(z0 + dz);
    };
    const uint4 *body = reinterpret_cast<const uint4 *>(base + (size_t)head * ES);
    auto visit = [&](const uint4 v, uint32_t p) {
      if ((v.x | v.y | v.z | v.w) == 0) return;
      uint32_t m = region_nonzero_bits<ES, FLOATBITS>(v);
      if (m == 0) return;  // -0.0f only
      acc.count += __popc(m);
      uint32_t x, y, z;
      locate(head + p * EPP, x, y, z);
      if (x + EPP <= nx) {  // the piece lies in one row
        acc.add(x + (uint32_t)__ffs(m) - 1u, y, z);
        acc.add(x + 31u - (uint32_t)__clz(m), y, z);
      } else {
        for (uint32_t i = 0; i < EPP; ++i) {
          if ((m >> i) & 1u) acc.add(x, y, z);
          if (++x == nx) {
            x = 0;
            if (++y == ny) { y = 0; ++z; }
          }
        }
      }
    };
    // four loads in flight per lane, then the four pieces; what is left of the unit one by one
    uint32_t p0 = 0;
    for (; npieces - p0 >= 4 * REGION_BLOCK; p0 += 4 * REGION_BLOCK) {
      uint4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = body[p0 + j * REGION_BLOCK + threadIdx.x];
#pragma unroll
      for (int j = 0; j < 4; ++j) visit(v[j], p0 + j * REGION_BLOCK + threadIdx.x);
    }
    for (uint32_t p = p0 + threadIdx.x; p < npieces; p += REGION_BLOCK) visit(body[p], p);
    // the elements before the first and behind the last aligned piece: fewer than 2 * EPP
    if (threadIdx.x < 2 * EPP) {
      const bool at_tail = threadIdx.x >= EPP;
      const uint32_t e = at_tail ? tail0 + (threadIdx.x - EPP) : threadIdx.x;
      if (e < (at_tail ? nelem : head)) {
        uint32_t bits = 0;
        for (int b = 0; b < ES; ++b) bits |= (uint32_t)base[(size_t)e * ES + b] << (8 * b);
        if (FLOATBITS) bits &= 0x7fffffffu;
        if (bits) {
          uint32_t x, y, z;
          locate(e, x, y, z);
          acc.add(x, y, z);
          acc.count += 1;
        }
      }
    }
  }
  // across the wave, then across the waves through LDS; one update of the record per workgroup
  for (int off = 32; off > 0; off >>= 1) {
    for (int a = 0; a < 3; ++a) {
      acc.lo[a] = min(acc.lo[a], (uint32_t)__shfl_xor((int)acc.lo[a], off));
      acc.hi[a] = max(acc.hi[a], (uint32_t)__shfl_xor((int)acc.hi[a], off));
    }
    acc.count += (unsigned long long)__shfl_xor((long long)acc.count, off);
  }
  __shared__ RegionBoxRecord part[REGION_WAVES];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    for (int a = 0; a < 3; ++a) { part[wave].lo[a] = acc.lo[a]; part[wave].hi[a] = acc.hi[a]; }
    part[wave].count = acc.count;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < REGION_WAVES; ++w) {
      for (int a = 0; a < 3; ++a) {
        acc.lo[a] = min(acc.lo[a], part[w].lo[a]);
        acc.hi[a] = max(acc.hi[a], part[w].hi[a]);
      }
      acc.count += part[w].count;
    }
    if (acc.count) {
      // Updates of one address from every workgroup queue behind each other.  A minimum only
      // falls and a maximum only rises, so a corner that a relaxed read already finds no worse
      // than ours needs no update, however stale the read is.
      for (int a = 0; a < 3; ++a) {
        if (__hip_atomic_load(&rec->lo[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > acc.lo[a])
          atomicMin(&rec->lo[a], acc.lo[a]);
        if (__hip_atomic_load(&rec->hi[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < acc.hi[a])
          atomicMax(&rec->hi[a], acc.hi[a]);
      }
      atomicAdd(&rec->count, acc.count);
    }
  }
}

// ---- extract ----------------------------------------------------------------------------------
struct RegionExtractArgs {
  RegionAxis ax[3];       // region_plan.hpp: x, y, z
  int64_t out_n[3];       // the output's size
  int64_t src_nx, src_ny;
  uint4 pad;              // the pad element repeated over 16 bytes
};

// the elements of a piece in reverse order
template <int ES>
__device__ inline uint4 region_reverse(const uint4 v) {
  if (ES == 8) return make_uint4(v.z, v.w, v.x, v.y);
  if (ES == 4) return make_uint4(v.w, v.z, v.y, v.x);
  if (ES == 2)
    return make_uint4((v.w >> 16) | (v.w << 16), (v.z >> 16) | (v.z << 16), (v.y >> 16) | (v.y << 16),
                      (v.x >> 16) | (v.x << 16));
  return make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x));
}

template <int ES> struct RegionElem;
template <> struct RegionElem<1> { typedef uint8_t type; };
template <> struct RegionElem<2> { typedef uint16_t type; };
template <> struct RegionElem<4> { typedef uint32_t type; };
template <> struct RegionElem<8> { typedef uint64_t type; };

// A wave takes an output row.  The row's aligned 16-byte pieces fall into five uniform runs:
// [pad | edge | copy | edge | pad]; the pad and copy runs are loops without a condition on their
// memory operations, the edges (at most one piece each) and the row's head and tail, short of a
// piece, go element by element.  The source of a copied piece starts at any byte offset; with
// FLIPX it is read from its lowest address and reversed.
template <int ES, bool FLIPX>
__global__ __launch_bounds__(REGION_BLOCK) void region_extract_kernel(const unsigned char *__restrict__ src,
                                                                       unsigned char *__restrict__ dst,
                                                                       const RegionExtractArgs g, int64_t nrows) {
  typedef typename RegionElem<ES>::type T;
  constexpr int64_t EPP = 16 / ES;
  const int lane = threadIdx.x & 63;
  const int64_t sx = g.out_n[0];
  const T pad1 = *reinterpret_cast<const T *>(&g.pad);
  const int64_t stride = (int64_t)gridDim.x * REGION_WAVES;
  for (int64_t r = (int64_t)blockIdx.x * REGION_WAVES + (threadIdx.x >> 6); r < nrows; r += stride) {
    const int64_t oz = r / g.out_n[1], oy = r - oz * g.out_n[1];
    const int64_t ky = oy - g.ax[1].lo, kz = oz - g.ax[2].lo;
    const bool pad_row = ky < 0 || ky >= g.ax[1].n || kz < 0 || kz >= g.ax[2].n;
    // a row of pad has an empty copy run and no source address
    const int64_t lo = pad_row ? sx : g.ax[0].lo, n = pad_row ? 0 : g.ax[0].n;
    const unsigned char *srow = src;
    if (!pad_row)
      srow += (size_t)(((g.ax[2].src0 + kz * g.ax[2].step) * g.src_ny + (g.ax[1].src0 + ky * g.ax[1].step)) *
                       g.src_nx) * ES;
    unsigned char *drow = dst + (size_t)r * (size_t)sx * ES;
    const int64_t head = min(sx, (int64_t)((0 - reinterpret_cast<uintptr_t>(drow)) & 15u) / ES);
    const int64_t nb = (sx - head) / EPP;
    const int64_t a = lo - head, b = lo + n - head;
    int64_t k1 = a <= 0 ? 0 : a / EPP, k2 = a <= 0 ? 0 : (a + EPP - 1) / EPP;
    int64_t k3 = b <= 0 ? 0 : b / EPP, k4 = b <= 0 ? 0 : (b + EPP - 1) / EPP;
    k1 = min(k1, nb);
    k2 = min(k2, nb);
    k3 = min(max(k3, k2), nb);
    k4 = min(max(k4, k3), nb);
    uint4 *dpieces = reinterpret_cast<uint4 *>(drow + (size_t)head * ES);
    for (int64_t k = lane; k < k1; k += 64) dpieces[k] = g.pad;
    for (int64_t k = k4 + lane; k < nb; k += 64) dpieces[k] = g.pad;
    // source element of output element e of the copy run: src0 + (e - lo) * step
    // (a piece of the copy run never reaches below source element 0 or beyond the row's last)
    if (FLIPX) {
      const int64_t c = g.ax[0].src0 - (head - lo) - (EPP - 1);  // lowest source element of piece 0
      for (int64_t k = k2 + lane; k < k3; k += 64)
        dpieces[k] = region_reverse<ES>(region_load16(srow + (size_t)(c - k * EPP) * ES));
    } else {
      const int64_t c = g.ax[0].src0 + (head - lo);
      for (int64_t k = k2 + lane; k < k3; k += 64) dpieces[k] = region_load16(srow + (size_t)(c + k * EPP) * ES);
    }
    // the four short runs of elements: head, the two edge pieces, tail; 16 lanes each
    {
      const int which = lane >> 4;
      const int64_t i = lane & 15;
      const int64_t e0 = which == 0 ? 0 : which == 1 ? head + k1 * EPP : which == 2 ? head + k3 * EPP : head + nb * EPP;
      const int64_t e1 = which == 0 ? head : which == 1 ? head + k2 * EPP : which == 2 ? head + k4 * EPP : sx;
      const int64_t e = e0 + i;
      if (e < e1) {
        T v = pad1;
        if (e >= lo && e < lo + n)
          v = reinterpret_cast<const T *>(srow)[g.ax[0].src0 + (e - lo) * g.ax[0].step];
        reinterpret_cast<T *>(drow)[e] = v;
      }
    }
  }
}

// ---- membership -----------------------------------------------------------------------------
// bitmap: bit l set where label l is in the set; 2048 words (uint16) or 8 (uint8), copied to LDS
// once per workgroup.  The steady part takes 16 labels (uint8) or 8 (uint16) per 16-byte load from
// any byte offset and stores aligned pieces; the ends of `out` short of a piece go one by one.
template <typename T>
__global__ __launch_bounds__(REGION_BLOCK) void region_member_kernel(const T *__restrict__ labels, int64_t n,
                                                                      const uint32_t *__restrict__ bitmap, T inside,
                                                                      T outside, T *__restrict__ out) {
  constexpr int ES = sizeof(T), EPP = 16 / ES, WORDS = ES == 1 ? 8 : 2048;
  __shared__ uint32_t set[WORDS];
  for (int i = threadIdx.x; i < WORDS; i += REGION_BLOCK) set[i] = bitmap[i];
  __syncthreads();
  auto member = [&](uint32_t l) -> uint32_t { return ((set[l >> 5] >> (l & 31)) & 1u) ? inside : outside; };
  const int64_t head = min(n, (int64_t)((0 - reinterpret_cast<uintptr_t>(out)) & 15u) / ES);
  const int64_t npieces = (n - head) / EPP, tail0 = head + npieces * EPP;
  const unsigned char *s = reinterpret_cast<const unsigned char *>(labels + head);
  uint4 *d = reinterpret_cast<uint4 *>(out + head);
  const int64_t stride = (int64_t)gridDim.x * REGION_BLOCK;
  for (int64_t p = (int64_t)blockIdx.x * REGION_BLOCK + threadIdx.x; p < npieces; p += stride) {
    const uint4 v = region_load16(s + (size_t)p * 16);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ES == 1)
        o[j] = member(w[j] & 0xffu) | (member((w[j] >> 8) & 0xffu) << 8) | (member((w[j] >> 16) & 0xffu) << 16) |
               (member(w[j] >> 24) << 24);
      else
        o[j] = member(w[j] & 0xffffu) | (member(w[j] >> 16) << 16);
    }
    d[p] = make_uint4(o[0], o[1], o[2], o[3]);
  }
  if (blockIdx.x == 0 && threadIdx.x < 2 * EPP) {
    const bool at_tail = threadIdx.x >= EPP;
    const int64_t e = at_tail ? tail0 + (threadIdx.x - EPP) : threadIdx.x;
    if (e < (at_tail ? n : head)) out[e] = (T)member(labels[e]);
  }
}

#endif  // IFE_REGION_KERNELS_HPP
