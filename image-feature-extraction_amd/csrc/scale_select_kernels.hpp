// scale_select_kernels.hpp -- the kernel of ife_scale_select (include/ife_hip.h "scale selection",
// DESIGN.md section 4 "Scale selection").
//
//   scale_fold_kernel<FIRST, INDEX>   one scale folded into the running maximum of every measure.
//     A lane takes four consecutive voxels: the ev1, ev2, ev3 and LoG planes of the scale once,
//     every requested measure evaluated from that one read, response[m] and scale_index[m]
//     updated where the scale's response is strictly larger.  FIRST (scale 0) starts from
//     (0, 255) without reading the outputs, so nothing is cleared beforehand; INDEX: the scale
//     indices are kept.  Pointwise and memory-bound: no LDS, no barrier, no atomic.
//     Each array is read and written 16 bytes per lane (the indices 4) where its address at the
//     lane's first voxel allows it -- one bit of `vec` per array, decided on the host
//     (scale_select_capi.inc), the same for every lane -- and element by element otherwise, as is
//     the last, partial group of a volume whose voxel count is no multiple of four.
//     One group per lane, no grid-stride loop and no grid cap (launch_prep's shape).
#ifndef IFE_SCALE_SELECT_KERNELS_HPP
#define IFE_SCALE_SELECT_KERNELS_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "feature_kernels.hpp"  // f32x4
#include "scale_select_plan.hpp"

namespace ife {

// bits of `vec`
constexpr int SELECT_VEC_PLANE = 0;      // + 0 .. 3: ev1, ev2, ev3, LoG
constexpr int SELECT_VEC_RESPONSE = 4;   // + measure
constexpr int SELECT_VEC_INDEX = 8;      // + measure

struct SelectPlanes {
  const float *e1, *e2, *e3, *lap;  // components 2, 3, 4, 5 of one planar scale
};

// elements [i, i + 4) of p where they lie below n; vec: all four do and p + i is 16-byte aligned
__device__ __forceinline__ void select_load4(const float *__restrict__ p, int64_t i, int64_t n, bool vec, float v[4]) {
  if (vec) {
    const f32x4 t = *reinterpret_cast<const f32x4 *>(p + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? p[i + j] : 0.0f;
  }
}

__device__ __forceinline__ void select_store4(float *__restrict__ p, int64_t i, int64_t n, bool vec, const float v[4]) {
  if (vec) {
    *reinterpret_cast<f32x4 *>(p + i) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = v[j];
  }
}

// The response of one measure at one voxel and scale, as include/ife_hip.h states it: float
// arithmetic, expf.  Every early 0 is a select, never a product, so that a NaN or an infinity of
// a term that does not count cannot leak into it.
__device__ __forceinline__ float select_response(const SelectMeasure &k, float e1, float e2, float e3, float lap) {
  if (k.kind == IFE_SS_LAPLACIAN) return k.sign * (k.w * lap);
  const float a1 = k.w * e3, a2 = k.w * e2, a3 = k.w * e1;
  const bool s1 = k.sign * a1 > 0.0f, s2 = k.sign * a2 > 0.0f, s3 = k.sign * a3 > 0.0f;
  const bool counts = k.kind == IFE_SS_TUBE ? (s2 && s3) : k.kind == IFE_SS_PLATE ? s3 : (s1 && s2 && s3);
  if (!counts) return 0.0f;
  const float ra2 = (a2 * a2) / (a3 * a3);
  const float rb2 = a2 == 0.0f ? 0.0f : (a1 * a1) / fabsf(a2 * a3);
  const float s2sum = (a1 * a1 + a2 * a2) + a3 * a3;
  const float A = expf(-(ra2 * k.ka)), B = expf(-(rb2 * k.kb)), C = 1.0f - expf(-(s2sum * k.kc));
  if (k.kind == IFE_SS_TUBE) return ((1.0f - A) * B) * C;
  if (k.kind == IFE_SS_PLATE) return (A * B) * C;
  return ((1.0f - A) * (1.0f - B)) * C;
}

template <bool FIRST, bool INDEX>
__global__ __launch_bounds__(256) void scale_fold_kernel(SelectPlanes p, int64_t nvox, SelectMeasures ms, int scale,
                                                         uint32_t vec, float *__restrict__ response,
                                                         uint8_t *__restrict__ index) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= nvox) return;
  const bool full = i + 4 <= nvox;
  float e1[4], e2[4], e3[4], lap[4];
  select_load4(p.e1, i, nvox, full && (vec >> (SELECT_VEC_PLANE + 0) & 1u), e1);
  select_load4(p.e2, i, nvox, full && (vec >> (SELECT_VEC_PLANE + 1) & 1u), e2);
  select_load4(p.e3, i, nvox, full && (vec >> (SELECT_VEC_PLANE + 2) & 1u), e3);
  select_load4(p.lap, i, nvox, full && (vec >> (SELECT_VEC_PLANE + 3) & 1u), lap);
#pragma unroll
  for (int m = 0; m < IFE_SS_MAX_MEASURES; ++m) {
    if (m >= ms.n) break;  // the same for every lane
    const SelectMeasure k = ms.m[m];
    float *resp = response + (int64_t)m * nvox;
    uint8_t *idx = INDEX ? index + (int64_t)m * nvox : nullptr;
    const bool rvec = full && (vec >> (SELECT_VEC_RESPONSE + m) & 1u);
    const bool ivec = full && (vec >> (SELECT_VEC_INDEX + m) & 1u);
    float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t at[4] = {255u, 255u, 255u, 255u};
    if (!FIRST) {
      select_load4(resp, i, nvox, rvec, best);
      if (INDEX) {
        if (ivec) {
          const uint32_t t = *reinterpret_cast<const uint32_t *>(idx + i);
          at[0] = t & 255u; at[1] = t >> 8 & 255u; at[2] = t >> 16 & 255u; at[3] = t >> 24;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j < nvox) at[j] = idx[i + j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float r = select_response(k, e1[j], e2[j], e3[j], lap[j]);
      if (r > best[j]) {  // strictly: the first of equal scales stays, a NaN never enters
        best[j] = r;
        at[j] = (uint32_t)scale;
      }
    }
    select_store4(resp, i, nvox, rvec, best);
    if (INDEX) {
      if (ivec) {
        *reinterpret_cast<uint32_t *>(idx + i) = at[0] | at[1] << 8 | at[2] << 16 | at[3] << 24;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i + j < nvox) idx[i + j] = (uint8_t)at[j];
      }
    }
  }
}

}  // namespace ife

#endif  // IFE_SCALE_SELECT_KERNELS_HPP
