// iir_kernels.inc -- ITK's 4th-order recursive (Deriche) Gaussian as line kernels.
//
// Restates, per line, itk::RecursiveSeparableImageFilter::FilterDataArray with the
// ZeroOrder coefficients of itk::RecursiveGaussianImageFilter, which the reference
// reaches through NormalizedGaussianConvolutionImageFilter.hxx:51-55
// (SmoothingRecursiveGaussianImageFilter: axis order Z, X, Y; float images between
// axes; double line state).  SURVEY.md section 8 row a4.
//
// Mapping to the machine: one line per lane, 64 adjacent lines per wave.  A line is
// walked in register blocks of K samples.
//   forward sweep : causal recursion; three samples into every pair of blocks the four
//                   newest causal values (double) are written to a checkpoint array
//                   (32 B per line per 2K samples).
//   backward sweep: per pair, reload the checkpoint -- it IS the causal value of the
//                   pair's first three samples, and the x history behind it is those
//                   samples --, recompute the other 2K-3 causal values, run the
//                   anticausal recursion over the same 2K samples, and store
//                   float(causal + anticausal).  The line's last pair, where the sweep
//                   turns, takes its state from the forward sweep in registers.
// This keeps the exact sequential double arithmetic of the reference (every
// multiply and add rounds separately: the TU is built with -ffp-contract=off) while
// the only extra HBM traffic is the checkpoint array.  The causal partial sums never
// leave registers.
//
// Axis variants:
//   strided (Z, Y): lanes own adjacent x, samples are `sstride` elements apart;
//                   every load/store of a wave is one contiguous 256-B row.
//   contig (X)    : lines are contiguous in memory; a wave stages 64 lines x K
//                   samples through LDS (16-B global accesses, transposed so that a
//                   lane again owns one line).
#include <hip/hip_runtime.h>
#include <stdint.h>

// This file is included twice by ife_capi.hip, with IFE_IIR_NS / IFE_IIR_FMA set:
//   ife::iir_exact (IFE_IIR_FMA 0): every multiply and add rounds separately -- the
//                  arithmetic of the reference, and the default;
//   ife::iir_fma   (IFE_IIR_FMA 1): the same expressions with each a*b+c fused.  Opt-in
//                  (IFE_OPT_IIR_FMA): results differ from the exact build in the last
//                  double bit, i.e. by one float ulp at about one output in 10^8, which
//                  a second difference can amplify beyond the 1e-5 bar at those voxels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stddef.h>

#include <type_traits>

#include "iir_types.hpp"

#if IFE_IIR_FMA
#define IFE_MADD(a, b, acc) fma((a), (b), (acc))
#else
#define IFE_MADD(a, b, acc) ((a) * (b) + (acc))
#endif

namespace ife {
namespace IFE_IIR_NS {




// The twelve coefficients of the interior recursion: what a steady loop keeps in scalar
// registers.  The eight border coefficients (BN*, BM*) are read from the job where a border
// block runs (edge_coefs), so that they do not occupy 16 scalar registers along the whole line.
struct IirCoefMain {
  double N0, N1, N2, N3;
  double D1, D2, D3, D4;
  double M1, M2, M3, M4;
};
__device__ __forceinline__ IirCoefMain main_coefs(const IirCoef &c) {
  return IirCoefMain{c.N0, c.N1, c.N2, c.N3, c.D1, c.D2, c.D3, c.D4, c.M1, c.M2, c.M3, c.M4};
}
// all twenty, re-read from the kernel-argument segment (IirJobs is the first argument of
// every line kernel) at the point of use: the empty asm keeps the scalar loads from being
// lifted out of the rare path that needs them.  (Taking the address of the by-value argument
// instead would make the compiler copy all of it to scratch memory.)
__device__ __forceinline__ IirCoef edge_coefs(uint32_t job) {
  typedef __attribute__((address_space(4))) const char kchar;
  kchar *ka = (kchar *)__builtin_amdgcn_kernarg_segment_ptr() + (size_t)job * sizeof(IirJob) + offsetof(IirJob, c);
  asm volatile("" : "+s"(ka));
  typedef __attribute__((address_space(4))) const double kdouble;
  kdouble *d = (kdouble *)ka;
  IirCoef r;
  r.N0 = d[0]; r.N1 = d[1]; r.N2 = d[2]; r.N3 = d[3];
  r.D1 = d[4]; r.D2 = d[5]; r.D3 = d[6]; r.D4 = d[7];
  r.M1 = d[8]; r.M2 = d[9]; r.M3 = d[10]; r.M4 = d[11];
  r.BN1 = d[12]; r.BN2 = d[13]; r.BN3 = d[14]; r.BN4 = d[15];
  r.BM1 = d[16]; r.BM2 = d[17]; r.BM3 = d[18]; r.BM4 = d[19];
  return r;
}
static_assert(sizeof(IirCoef) == 20 * sizeof(double), "edge_coefs reads IirCoef as 20 doubles");

struct CausalState {
  double x1, x2, x3;      // x[i-1], x[i-2], x[i-3]
  double y1, y2, y3, y4;  // y[i-1..i-4]
};
struct AntiState {
  double x1, x2, x3, x4;  // x[i+1..i+4]
  double y1, y2, y3, y4;  // y[i+1..i+4]
};

// scratch[i] = data[i]*N0 + data[i-1]*N1 + data[i-2]*N2 + data[i-3]*N3
// scratch[i] -= scratch[i-1]*D1 + scratch[i-2]*D2 + scratch[i-3]*D3 + scratch[i-4]*D4
template <typename C>
__device__ __forceinline__ double causal_step(CausalState &s, double xin, const C &c) {
  const double a = IFE_MADD(s.x3, c.N3, IFE_MADD(s.x2, c.N2, IFE_MADD(s.x1, c.N1, xin * c.N0)));
  const double t = IFE_MADD(s.y4, c.D4, IFE_MADD(s.y3, c.D3, IFE_MADD(s.y2, c.D2, s.y1 * c.D1)));
  const double y = a - t;
  s.x3 = s.x2; s.x2 = s.x1; s.x1 = xin;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
  return y;
}
// Border form: for i < 4 the taps that reach before the line use outV1*BN_k, which is
// what the state holds (y_k initialised to outV1) times the boundary coefficient.
__device__ __forceinline__ double causal_step_edge(CausalState &s, double xin, const IirCoef &c,
                                                   int64_t i) {
  const double d1 = i < 1 ? c.BN1 : c.D1;
  const double d2 = i < 2 ? c.BN2 : c.D2;
  const double d3 = i < 3 ? c.BN3 : c.D3;
  const double d4 = i < 4 ? c.BN4 : c.D4;
  const double a = IFE_MADD(s.x3, c.N3, IFE_MADD(s.x2, c.N2, IFE_MADD(s.x1, c.N1, xin * c.N0)));
  const double t = IFE_MADD(s.y4, d4, IFE_MADD(s.y3, d3, IFE_MADD(s.y2, d2, s.y1 * d1)));
  const double y = a - t;
  s.x3 = s.x2; s.x2 = s.x1; s.x1 = xin;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
  return y;
}
// scratch[i] = data[i+1]*M1 + data[i+2]*M2 + data[i+3]*M3 + data[i+4]*M4
// scratch[i] -= scratch[i+1]*D1 + scratch[i+2]*D2 + scratch[i+3]*D3 + scratch[i+4]*D4
template <typename C>
__device__ __forceinline__ double anti_step(AntiState &s, double xin, const C &c) {
  const double a = IFE_MADD(s.x4, c.M4, IFE_MADD(s.x3, c.M3, IFE_MADD(s.x2, c.M2, s.x1 * c.M1)));
  const double t = IFE_MADD(s.y4, c.D4, IFE_MADD(s.y3, c.D3, IFE_MADD(s.y2, c.D2, s.y1 * c.D1)));
  const double y = a - t;
  s.x4 = s.x3; s.x3 = s.x2; s.x2 = s.x1; s.x1 = xin;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
  return y;
}
__device__ __forceinline__ double anti_step_edge(AntiState &s, double xin, const IirCoef &c,
                                                 int64_t i, int64_t n) {
  const double d1 = i + 1 >= n ? c.BM1 : c.D1;
  const double d2 = i + 2 >= n ? c.BM2 : c.D2;
  const double d3 = i + 3 >= n ? c.BM3 : c.D3;
  const double d4 = i + 4 >= n ? c.BM4 : c.D4;
  const double a = IFE_MADD(s.x4, c.M4, IFE_MADD(s.x3, c.M3, IFE_MADD(s.x2, c.M2, s.x1 * c.M1)));
  const double t = IFE_MADD(s.y4, d4, IFE_MADD(s.y3, d3, IFE_MADD(s.y2, d2, s.y1 * d1)));
  const double y = a - t;
  s.x4 = s.x3; s.x3 = s.x2; s.x2 = s.x1; s.x1 = xin;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
  return y;
}

// ---- addressing ------------------------------------------------------------------
// Every global access below is a raw buffer access: a wave-uniform 128-bit resource
// (base pointer rebuilt per register block from scalars), a constant 32-bit per-lane
// byte offset, and a scalar per-sample offset.  The per-sample address arithmetic is
// scalar, no 64-bit address lives in VGPRs, and SGPR pressure stays at one resource
// per stream (the 20 double coefficients already take 40 SGPRs).
using rsrc_t = __amdgpu_buffer_rsrc_t;

__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ rsrc_t make_rsrc(const void *ubase) {
  // stride 0, no range limit: offsets are validated on the host (ife_capi.hip)
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(ubase), 0, -1, 0x00020000);
}
// Timing-only diagnostics (MI355X guide, "price ONE buffer's traffic"): a resource with zero
// records drops every access through it while the instruction stream stays.  Never defined
// in the product build; results are wrong by construction.
__device__ __forceinline__ rsrc_t make_rsrc_null(const void *ubase) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(ubase), 0, 0, 0x00020000);
}
// A descriptor whose byte range is a scalar the caller has computed with INTEGER arithmetic
// (0xffffffff: unbounded, 0: every access through it is dropped).  Not a bool: a condition
// carried as an i1 may end up as a lane mask, the select then runs on the vector unit and the
// compiler loops over the "distinct" descriptors at every use.
__device__ __forceinline__ rsrc_t make_rsrc_range(const void *ubase, uint32_t range) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(ubase), 0, (int)range, 0x00020000);
}
// all ones where a < b (signed, wave-uniform, no overflow), else 0.  In assembly because the
// compiler rewrites (a - b) >> 31 into select(a < b, -1, 0), whose condition it then keeps as a
// lane mask: exactly the vector-unit select this is here to avoid.
__device__ __forceinline__ uint32_t mask_lt(int a, int b) {
  uint32_t m;
  asm("s_sub_i32 %0, %1, %2\n\ts_ashr_i32 %0, %0, 31" : "=s"(m) : "s"(a), "s"(b) : "scc");
  return m;
}
#if defined(IFE_DIAG_NO_OUT)
#define IFE_OUT_RSRC make_rsrc_null
#define IFE_OUT_RSRC_RANGE(ptr, range) make_rsrc_null(ptr)
#else
#define IFE_OUT_RSRC make_rsrc
#define IFE_OUT_RSRC_RANGE(ptr, range) make_rsrc_range((ptr), (range))
#endif
#if defined(IFE_DIAG_NO_CK)
#define IFE_CK_RSRC make_rsrc_null
#else
#define IFE_CK_RSRC make_rsrc
#endif
#if defined(IFE_DIAG_NO_IN)
#define IFE_IN_RSRC make_rsrc_null
#else
#define IFE_IN_RSRC make_rsrc
#endif
__device__ __forceinline__ float buf_ld_f32(rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
// The backward sweep's loads are the LAST use of the input in this launch.
#ifndef IFE_IN2_AUX
#define IFE_IN2_AUX 0
#endif
__device__ __forceinline__ float buf_ld_last_f32(rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, IFE_IN2_AUX));
}
__device__ __forceinline__ void buf_st_f32(rsrc_t r, uint32_t voff, uint32_t soff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, 0);
}
// Stores of a pass's OUTPUT: nothing in this launch reads them again, while its input is read
// a second time by the backward sweep; cache-policy bits (2 = nt) let the output stream past.
#ifndef IFE_OUT_AUX
#define IFE_OUT_AUX 2  // measured: x 2.27 -> 2.20 ms, y 2.02 -> 1.96 ms
#endif
__device__ __forceinline__ void buf_st_out_f32(rsrc_t r, uint32_t voff, uint32_t soff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, IFE_OUT_AUX);
}
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// Checkpoints are written by the forward sweep and read once by the backward sweep, a whole
// line later: cache-policy bits for both (0 default, 1 sc0, 2 nt, 3 sc0+nt; experiments README)
#ifndef IFE_CK_ST_AUX
#define IFE_CK_ST_AUX 0
#endif
#ifndef IFE_CK_LD_AUX
#define IFE_CK_LD_AUX 0
#endif
__device__ __forceinline__ double ck_ld_f64(rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, IFE_CK_LD_AUX));
}
__device__ __forceinline__ void ck_st_f64(rsrc_t r, uint32_t voff, uint32_t soff, double v) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, soff, IFE_CK_ST_AUX);
}
__device__ __forceinline__ float ck_ld_f32(rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, IFE_CK_LD_AUX));
}
__device__ __forceinline__ void ck_st_f32(rsrc_t r, uint32_t voff, uint32_t soff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, IFE_CK_ST_AUX);
}
__device__ __forceinline__ double buf_ld_f64(rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ __forceinline__ void buf_st_f64(rsrc_t r, uint32_t voff, uint32_t soff, double v) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, soff, 0);
}
template <typename T>
__device__ __forceinline__ float buf_ld_as_f32(rsrc_t r, uint32_t voff, uint32_t soff);
template <>
__device__ __forceinline__ float buf_ld_as_f32<float>(rsrc_t r, uint32_t voff, uint32_t soff) {
  return buf_ld_f32(r, voff, soff);
}
template <>
__device__ __forceinline__ float buf_ld_as_f32<uint8_t>(rsrc_t r, uint32_t voff, uint32_t soff) {
  return (float)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(r, voff, soff, 0);
}
template <>
__device__ __forceinline__ float buf_ld_as_f32<uint16_t>(rsrc_t r, uint32_t voff, uint32_t soff) {
  return (float)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0);
}
template <>
__device__ __forceinline__ float buf_ld_as_f32<int16_t>(rsrc_t r, uint32_t voff, uint32_t soff) {
  return (float)(int16_t)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0);
}

// ---- constant lines (IirJob::const_lines, set by the host: ife_capi.hip const_line_flags) ----
// Bit patterns, not values: +0 and -0 are different constants here (the filter may answer a
// line of -0 with +0), so that the shortcut leaves the sign of a zero exactly as the recursion
// would.  Returns whether a line made of `bits` may be answered with a constant, and which.
__device__ __forceinline__ bool const_line_response(uint32_t bits, uint32_t flags, float &resp) {
  resp = __builtin_bit_cast(float, bits);
  if (bits == 0u) return (flags & 1u) != 0;
  if (bits == 0x3f800000u) return (flags & 2u) != 0;
  if (bits == 0x80000000u) {
    if (flags & 8u) resp = 0.0f;
    return (flags & 12u) != 0;
  }
  return false;
}
__device__ __forceinline__ bool same_bits(float a, float b) {
  return __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b);
}

// ---- jobs ------------------------------------------------------------------------
// One launch runs up to IIR_MAX_JOBS independent line filters of the same geometry
// (numerator and denominator of up to three scales): iir_block_of selects the job.  All
// line kernels read and write float volumes (the cast/multiply prepass feeds the first).

struct SrcF32 {
  const float *p;
  struct At { rsrc_t a; };
  __device__ __forceinline__ At at(int64_t u) const { return At{IFE_IN_RSRC(p + u)}; }
  // range 0: an empty descriptor -- the loads through it are issued and dropped
  __device__ __forceinline__ At at(int64_t u, uint32_t range) const { return At{make_rsrc_range(p + u, range)}; }
#if defined(IFE_DIAG_BYTE_LOADS)
  // timing only (wrong results): the same addresses (1) or a quarter of the footprint (2)
  // through byte-wide loads -- what a mask read in place by the line kernel would cost
  __device__ __forceinline__ float ld(const At &b, uint32_t v, uint32_t s) const {
    constexpr uint32_t E = IFE_DIAG_BYTE_LOADS == 1 ? 4u : 1u;
    return (float)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(b.a, v * E, s * E, 0);
  }
  __device__ __forceinline__ float ld_last(const At &b, uint32_t v, uint32_t s) const { return ld(b, v, s); }
#else
  __device__ __forceinline__ float ld(const At &b, uint32_t v, uint32_t s) const {
    return buf_ld_f32(b.a, v * 4u, s * 4u);
  }
  __device__ __forceinline__ float ld_last(const At &b, uint32_t v, uint32_t s) const {
    return buf_ld_last_f32(b.a, v * 4u, s * 4u);
  }
#endif
};

struct Checkpoint {
  double *y;
};

// The recursion state is saved once per PAIR of register blocks (every 2K samples), behind
// the pair's third sample i0+2: y1..y4 = y[i0+2], y[i0+1], y[i0], y[i0-1].  The x history
// that belongs to it is x[i0+2..i0], samples of the pair itself, so nothing in front of the
// pair is read again, and the first three causal values of the pair are not recomputed: they
// are y3, y2, y1, the very doubles the recomputation would produce.  That is 32 B per line
// per 2K samples each way, for the strided and the contiguous kernel alike.
__device__ __forceinline__ void ck_store(const Checkpoint &ck, int64_t pair, int64_t nl,
                                         int64_t Lw, uint32_t lane, const CausalState &s) {
  const rsrc_t ry = IFE_CK_RSRC(ck.y + (pair * 4) * nl + Lw);
  const uint32_t sy = (uint32_t)nl * 8u;
  ck_st_f64(ry, lane * 8u, 0u, s.y1);
  ck_st_f64(ry, lane * 8u, sy, s.y2);
  ck_st_f64(ry, lane * 8u, 2u * sy, s.y3);
  ck_st_f64(ry, lane * 8u, 3u * sy, s.y4);
}
__device__ __forceinline__ void ck_load(const Checkpoint &ck, int64_t pair, int64_t nl,
                                        int64_t Lw, uint32_t lane, CausalState &s) {
  const rsrc_t ry = IFE_CK_RSRC(ck.y + (pair * 4) * nl + Lw);
  const uint32_t sy = (uint32_t)nl * 8u;
  s.y1 = ck_ld_f64(ry, lane * 8u, 0u);
  s.y2 = ck_ld_f64(ry, lane * 8u, sy);
  s.y3 = ck_ld_f64(ry, lane * 8u, 2u * sy);
  s.y4 = ck_ld_f64(ry, lane * 8u, 3u * sy);
}

// The first block of a pair is run twice from the same state (once to reach the second
// block, once for its own values).  Left alone, the compiler merges the two runs and keeps
// all K values of the first one alive across the second block: exactly the register
// footprint the recomputation is there to avoid.  Passing the state through an empty asm
// makes the second run opaque.
__device__ __forceinline__ void opaque_state(CausalState &s) {
  asm volatile("" : "+v"(s.y1), "+v"(s.y2), "+v"(s.y3), "+v"(s.y4));
}

// Causal recursion over one register block starting at sample i0.  `edge` blocks (the
// first one, and any block that may run past the line end) take the border form and skip
// samples >= n.  STORE keeps the K values for the anticausal pass.
template <int K, bool STORE>
__device__ __forceinline__ void causal_run(CausalState &s, const float (&x)[K], double (&cz)[K],
                                           const IirCoef &c, int64_t i0, int64_t n, bool edge) {
  if (!edge) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double y = causal_step(s, (double)x[j], c);
      if (STORE) cz[j] = y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (i0 + j < n) {
        const double y = causal_step_edge(s, (double)x[j], c, i0 + j);
        if (STORE) cz[j] = y;
      }
  }
}
// The causal values of the FIRST block of a pair are parked in LDS while the second block
// runs (a lane only ever touches its own column: the strip is private spill space, element
// j of lane l at [j][l], so every ds_write_b64 / ds_read_b64 is conflict-free and no
// synchronisation is needed).  Before this the first block was simply run twice; parking
// it takes the sweep from 3.5 to 3.0 recursion steps per sample without changing a rounding.
#ifndef IFE_IIR_LDS_CZ
#define IFE_IIR_LDS_CZ 1
#endif
template <int K>
__device__ __forceinline__ void causal_run_park(CausalState &s, const float (&x)[K], double *col,
                                                const IirCoef &c, int64_t i0, int64_t n, bool edge) {
  if (!edge) {
#pragma unroll
    for (int j = 0; j < K; ++j) col[j * 64] = causal_step(s, (double)x[j], c);
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (i0 + j < n) col[j * 64] = causal_step_edge(s, (double)x[j], c, i0 + j);
  }
}
template <int K>
__device__ __forceinline__ void causal_unpark(double (&cz)[K], const double *col) {
#pragma unroll
  for (int j = 0; j < K; ++j) cz[j] = col[j * 64];
}
// anti_run with the causal values read back from the lane's LDS column as they are needed
// (no K-wide register array for the parked block)
template <int K>
__device__ __forceinline__ void anti_run_parked(AntiState &a, float (&x)[K], const double *col,
                                                const IirCoef &c, int64_t i0, int64_t n, bool edge) {
  if (!edge) {
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
      const double y = anti_step(a, (double)x[j], c);
      x[j] = (float)(col[j * 64] + y);
    }
  } else {
#pragma unroll
    for (int j = K - 1; j >= 0; --j)
      if (i0 + j < n) {
        const double y = anti_step_edge(a, (double)x[j], c, i0 + j, n);
        x[j] = (float)(col[j * 64] + y);
      }
  }
}

// Anticausal recursion over the same block, leaving float(causal + anticausal) in x.
template <int K>
__device__ __forceinline__ void anti_run(AntiState &a, float (&x)[K], const double (&cz)[K],
                                         const IirCoef &c, int64_t i0, int64_t n, bool edge) {
  if (!edge) {
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
      const double y = anti_step(a, (double)x[j], c);
      x[j] = (float)(cz[j] + y);
    }
  } else {
#pragma unroll
    for (int j = K - 1; j >= 0; --j)
      if (i0 + j < n) {
        const double y = anti_step_edge(a, (double)x[j], c, i0 + j, n);
        x[j] = (float)(cz[j] + y);
      }
  }
}

// =================================================================================
// strided axes (Z and Y)
// =================================================================================
// PAIRED (last pass of the normalized convolution, NormalizedGaussianConvolutionImageFilter.
// hxx:51-61): a workgroup covers 128 lines; waves 0-1 run the numerator of those lines, waves
// 2-3 the denominator, each exactly as in the plain form.  Per block pair the denominator
// waves hand their float results to their sibling through LDS (their own parking strip is
// free by then) and the numerator waves store only the quotient, ITK's Div functor
// (B != 0 ? A / B : max).  The two fields this replaces were written here and read again by
// the feature kernel: 8 B per voxel and scale less HBM traffic at unchanged occupancy.
__device__ __forceinline__ void lds_workgroup_sync() {
  // LDS only: the global loads and stores in flight stay in flight across the barrier
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// Memory operations and waits.  The compiler places s_waitcnt vmcnt(N) from a model of what is
// outstanding, and where a load or store sits behind a branch it must assume the path with
// the fewest younger operations: N shrinks to what is certain and the wait drains more than
// it needs -- round 2's kernel, with its conditional prefetches and `if (live)` stores, waited
// for vmcnt(0) at the top of every forward iteration and at the bottom of every backward one,
// i.e. for the loads it had just issued and for its own output stores.  So the steady state
// below contains no conditional memory operation at all:
//   * a load that may not be needed goes through a descriptor whose size a scalar select has
//     set to zero (the access is dropped, the instruction and its place in the count stay);
//   * a lane past the last line repeats the last line -- same loads, same arithmetic, the same
//     values stored to the same addresses -- instead of being masked off;
//   * the pairs that touch an end of the line (border coefficients, ragged tail, no
//     predecessor) run through a general body outside the steady loop.
// The waits the compiler then emits are exact: the loads of a pair are consumed a whole pair
// after they were issued, and no store is ever waited for.
#ifndef IFE_IIR_FENCE
#define IFE_IIR_FENCE 2  // recursion steps between scheduling fences in the steady iteration
#endif
// BWD (first axis pass behind iir_sweep_z_kernel): no forward sweep here.  The checkpoints are
// in place, the state in front of the last pair is read from that pair's checkpoint slot, and
// the constant-line decision takes the forward half from the field's per-line record.
template <int K, bool PAIRED = false, bool BWD = false>
__global__ __launch_bounds__(256, K <= 10 ? 4 : (IFE_IIR_LDS_CZ && K <= 12 ? 3 : 1)) void iir_strided_kernel(IirJobs jobs, IirGeom g) {
  static_assert(!(PAIRED && BWD), "the backward-only form is the plain form of the first axis pass");
  const IirBlock blk = iir_block_of(g, blockIdx.x);
  if (!blk.live) return;
  const IirJob &J = jobs.j[blk.job];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool is_den = PAIRED && wave_id >= 2u;  // wave-uniform
  const uint32_t out_range = (wave_id >> 1) - 1u;  // paired: all ones for the numerator waves, 0 for the others
  const SrcF32 src{is_den ? J.in2 : J.in};
  float *__restrict__ out = J.out;
  const IirCoefMain c = main_coefs(J.c);  // interior recursion; border blocks read edge_coefs(blk.job)
  const Checkpoint ck{is_den ? J.ck_y2 : J.ck_y};
  int64_t Lw = PAIRED ? uniform64((int64_t)blk.group * 128 + (int64_t)(wave_id & 1u) * 64)
                      : uniform64((int64_t)blk.group * blockDim.x + (int64_t)(threadIdx.x & ~63u));
  const bool wave_dead = Lw >= g.nlines;
  if (!PAIRED && wave_dead) return;  // wave-uniform
  // PAIRED: every wave must reach the workgroup barriers; a wave without lines repeats the
  // first lines of the job (identical values to identical places, like a lane past the end)
  if (wave_dead) Lw = 0;
  const int64_t n = g.n, st = g.sstride, nl = g.nlines;
  int64_t L = Lw + lane;
  if (L >= nl) L = nl - 1;  // a lane past the last line repeats the last line
  const uint32_t cl = (uint32_t)(L - Lw);  // this lane's slot in the wave's checkpoint rows
  const int64_t base = (L % g.inner) + (L / g.inner) * g.outer;
  const int64_t wbase = uniform64(base);          // lane 0 of the wave
  const uint32_t voff = (uint32_t)(base - wbase);  // elements (one row jump at most)
  const uint32_t sst = (uint32_t)st;               // 2K*st*4 < 2^31 is checked on the host
  const int nb = (int)((n + K - 1) / K);            // register blocks
  const int np = (nb + 1) / 2;                      // block pairs (checkpoint granularity)
#if IFE_IIR_LDS_CZ
  __shared__ double park[4][2 * K][64];  // both blocks of a pair: no causal values in registers
  double *col = &park[threadIdx.x >> 6][0][lane];
#else
#error "the strided kernel parks the causal values of a pair in LDS"
#endif

  // ---------------- forward sweep: a checkpoint for every pair 1 .. np-2 ----------------
  // Pairs 0 .. np-2 (all complete; the last pair is only read by the backward sweep), two
  // pairs of samples in flight in two register sets.
  // Constant lines: every sample of the line equals its first one (tracked here for one
  // compare per sample) and that value may be copied (J.const_lines).  Decided per wave in
  // the backward sweep, once the last pair has been seen.
  bool fwd_const = true;
  float fwd_ref = 0.0f;
  // The state in front of the LAST pair never goes through memory: the forward sweep ends
  // there and the backward sweep starts there, so it is handed over in registers.
  CausalState turn;
  turn.x1 = turn.x2 = turn.x3 = 0.0;
  turn.y1 = turn.y2 = turn.y3 = turn.y4 = 0.0;
  if constexpr (!BWD) {
    float a0[K], a1[K], b0[K], b1[K];
    CausalState s;
    const int nfp = np - 1;
    auto load_pair_f = [&](int p, float (&u)[K], float (&v)[K]) {
      const auto B = src.at(wbase + (int64_t)(2 * p * K) * st, mask_lt(p, nfp));  // beyond the sweep: dropped
#pragma unroll
      for (int j = 0; j < K; ++j) u[j] = src.ld(B, voff, (uint32_t)j * sst);
#pragma unroll
      for (int j = 0; j < K; ++j) v[j] = src.ld(B, voff, (uint32_t)(K + j) * sst);
    };
    auto track = [&](const float (&x)[K]) {
      if constexpr (!PAIRED) {  // the paired form has no shortcut: its two waves meet at barriers
        if (J.const_lines) {
#pragma unroll
          for (int j = 0; j < K; ++j) fwd_const = fwd_const && same_bits(x[j], fwd_ref);
        }
      }
    };
    // pair p, 1 <= p <= np-2: its checkpoint is taken THREE samples into the pair (ck_store)
    auto run_pair = [&](int p, const float (&u)[K], const float (&v)[K]) {
#pragma unroll
      for (int j = 0; j < 3; ++j) causal_step(s, (double)u[j], c);
      ck_store(ck, p, nl, Lw, cl, s);
#pragma unroll
      for (int j = 3; j < K; ++j) causal_step(s, (double)u[j], c);
      track(u);
#pragma unroll
      for (int j = 0; j < K; ++j) causal_step(s, (double)v[j], c);
      track(v);
    };
    if (nfp > 0) {
      load_pair_f(0, a0, a1);
      load_pair_f(1, b0, b1);
      {  // pair 0: border form on the first four samples
        const double e0 = (double)a0[0];
        fwd_ref = a0[0];
        s.x1 = s.x2 = s.x3 = e0;
        s.y1 = s.y2 = s.y3 = s.y4 = e0;
        {
          const IirCoef ce = edge_coefs(blk.job);
#pragma unroll
          for (int j = 0; j < K; ++j) causal_step_edge(s, (double)a0[j], ce, j);
        }
        track(a0);
#pragma unroll
        for (int j = 0; j < K; ++j) causal_step(s, (double)a1[j], c);
        track(a1);
      }
      load_pair_f(2, a0, a1);
      int p = 1;  // b holds pair p, a holds pair p+1
      for (; p + 1 < nfp; p += 2) {
        run_pair(p, b0, b1);
        load_pair_f(p + 2, b0, b1);
        run_pair(p + 1, a0, a1);
        load_pair_f(p + 3, a0, a1);
      }
      if (p < nfp) run_pair(p, b0, b1);
      turn = s;
    }
  } else {
    // left by the shared sweep: y1..y4 in the checkpoint slot of the last pair; the x history
    // that belongs to them is the three samples in front of that pair
    if (np > 1) {
      ck_load(ck, np - 1, nl, Lw, cl, turn);
      const auto B = src.at(wbase + ((int64_t)(2 * (np - 1) * K) - 3) * st);
      turn.x3 = (double)src.ld(B, voff, 0u);
      turn.x2 = (double)src.ld(B, voff, sst);
      turn.x1 = (double)src.ld(B, voff, 2u * sst);
      // ZSWEEP_NOT_CONST where a sample in front of the last pair differs from the first one
      if (J.const_lines) fwd_ref = __builtin_bit_cast(float, J.line_rec[L]);
    }
  }

  // ---------------- backward sweep, one pair of blocks per iteration ----------------
  {
    float xa[K], xb[K];  // blocks 2p and 2p+1 of the current pair
    float na[K], nb2[K];  // the next pair (p-1), in flight
    AntiState a;
    auto load_pair = [&](int p, float (&pa)[K], float (&pb)[K], bool clampn) {
      const int64_t i0 = (int64_t)(2 * p * K);
      const auto B = src.at(wbase + i0 * st);
      if (!clampn) {
#pragma unroll
        for (int j = 0; j < K; ++j) pa[j] = src.ld_last(B, voff, (uint32_t)j * sst);
#pragma unroll
        for (int j = 0; j < K; ++j) pb[j] = src.ld_last(B, voff, (uint32_t)(K + j) * sst);
      } else {
        const uint32_t lastj = (uint32_t)(n - 1 - i0);  // 0 .. 2K-1
#pragma unroll
        for (int j = 0; j < K; ++j)
          pa[j] = src.ld_last(B, voff, ((uint32_t)j < lastj ? (uint32_t)j : lastj) * sst);
#pragma unroll
        for (int j = 0; j < K; ++j)
          pb[j] = src.ld_last(B, voff, ((uint32_t)(K + j) < lastj ? (uint32_t)(K + j) : lastj) * sst);
      }
    };
    // checkpoint of the current pair and, in flight, of the next one
    CausalState sc, sn;
    sc.y1 = sc.y2 = sc.y3 = sc.y4 = 0.0;
    sn = sc;
    load_pair(np - 1, xa, xb, true);
    // ---- constant lines: all 64 lines of the wave equal to 0 or (where allowed) 1 throughout ----
    bool wave_const = false;
    float cval = 0.0f;
    if (!PAIRED && J.const_lines) {  // uniform
      const float first = xa[0];
      bool cst = np == 1 || (fwd_const && same_bits(fwd_ref, first));
#pragma unroll
      for (int j = 0; j < K; ++j) cst = cst && same_bits(xa[j], first) && same_bits(xb[j], first);  // clamped slots repeat x[n-1]
      cst = const_line_response(__builtin_bit_cast(uint32_t, first), J.const_lines, cval) && cst;
      wave_const = __builtin_amdgcn_ballot_w64(!cst) == 0;
    }
    if (wave_const && !PAIRED) {
      // the filter answers these lines with the constant `cval`: nothing to read, nothing to compute
      for (int p = np - 1; p >= 0; --p) {
        const int64_t i0 = (int64_t)(2 * p * K);
        const rsrc_t ro = IFE_OUT_RSRC(out + wbase + i0 * st);
#pragma unroll
        for (int j = 0; j < 2 * K; ++j)
          if (i0 + j < n) buf_st_out_f32(ro, voff * 4u, (uint32_t)j * sst * 4u, cval);
      }
      return;
    }
    {
      // x[n-1]: the clamped loads make every slot past the line end hold it
      const double xN = (double)xb[K - 1];
      a.x1 = a.x2 = a.x3 = a.x4 = xN;
      a.y1 = a.y2 = a.y3 = a.y4 = xN;
    }
    // denominators of a block pair travel to the sibling wave through the denominator wave's
    // own parking strip, which is free once its anticausal values have been read
    float *fx = PAIRED ? reinterpret_cast<float *>(&park[is_den ? wave_id : wave_id + 2u][0][0]) + lane : nullptr;
    // the quotient of the normalized convolution (ITK's Div functor), numerator waves only
    auto quotient = [&](int64_t i0, int64_t i1) {
      // a wave whose denominators are all exactly one skips the division (A / 1 == A); slots
      // past the end of the line hold leftovers and are never stored.  The denominators are
      // read from the strip one at a time (twice where a division is needed) rather than held
      // in 2K registers next to the samples of two pairs.
      bool ones = true;
#pragma unroll
      for (int j = 0; j < K; ++j)
        ones = ones && (fx[j * 64] == 1.0f || i0 + j >= n) && (fx[(K + j) * 64] == 1.0f || i1 + j >= n);
      if (__builtin_amdgcn_ballot_w64(!ones) != 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const float da = fx[j * 64], db = fx[(K + j) * 64];
          xa[j] = da != 0.0f ? xa[j] / da : 3.402823466e+38f;
          xb[j] = db != 0.0f ? xb[j] / db : 3.402823466e+38f;
        }
      }
    };
    auto rotate = [&]() {
#pragma unroll
      for (int j = 0; j < K; ++j) { xa[j] = na[j]; xb[j] = nb2[j]; }
      sc.y1 = sn.y1; sc.y2 = sn.y2; sc.y3 = sn.y3; sc.y4 = sn.y4;
    };

    // ---- a pair away from both ends of the line whose predecessor has a checkpoint (p >= 2,
    // (2p+2)K + 4 <= n): no border form, no ragged block, every memory operation unconditional ----
    auto steady_iter = [&](int p) {
      const int64_t i0 = (int64_t)(2 * p * K);
      // the checkpoint IS the causal value of the pair's first three samples (and y[i0-1]),
      // and the x history behind it is the samples themselves
      CausalState s;
      s.y1 = sc.y1; s.y2 = sc.y2; s.y3 = sc.y3; s.y4 = sc.y4;
      s.x1 = (double)xa[2]; s.x2 = (double)xa[1]; s.x3 = (double)xa[0];
      col[0] = sc.y3; col[64] = sc.y2; col[128] = sc.y1;
      // (scheduling fences: left alone, the scheduler converts and loads far ahead across this
      // branch-free stretch and the allocation no longer fits four / three waves per SIMD)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 3; j < K; ++j) {
        col[j * 64] = causal_step(s, (double)xa[j], c);
        if (j % IFE_IIR_FENCE == IFE_IIR_FENCE - 1) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        col[(K + j) * 64] = causal_step(s, (double)xb[j], c);
        if (j % IFE_IIR_FENCE == IFE_IIR_FENCE - 1) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
      // the next pair is requested here, not at the top: it is only needed an iteration later,
      // and the causal half above is where the register demand peaks
      load_pair(p - 1, na, nb2, false);
      ck_load(ck, p - 1, nl, Lw, cl, sn);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        xb[j] = (float)(col[(K + j) * 64] + anti_step(a, (double)xb[j], c));
        if (j % IFE_IIR_FENCE == 0) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        xa[j] = (float)(col[j * 64] + anti_step(a, (double)xa[j], c));
        if (j % IFE_IIR_FENCE == 0) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (PAIRED) {
        if (is_den) {
#pragma unroll
          for (int j = 0; j < K; ++j) { fx[j * 64] = xa[j]; fx[(K + j) * 64] = xb[j]; }
        }
        lds_workgroup_sync();
        if (!is_den) quotient(i0, i0 + K);
      }
      // the denominator waves of the paired form issue the same stores through an empty
      // descriptor: every wave's operation count stays the same in every iteration
      const rsrc_t ro = PAIRED ? IFE_OUT_RSRC_RANGE(out + wbase + i0 * st, out_range) : IFE_OUT_RSRC(out + wbase + i0 * st);
#pragma unroll
      for (int j = 0; j < K; ++j) buf_st_out_f32(ro, voff * 4u, (uint32_t)(K + j) * sst * 4u, xb[j]);
#pragma unroll
      for (int j = 0; j < K; ++j) buf_st_out_f32(ro, voff * 4u, (uint32_t)j * sst * 4u, xa[j]);
      if constexpr (PAIRED) lds_workgroup_sync();  // the strip is parked into again in the next iteration
      rotate();
    };

    // ---- any pair: border forms at the line's ends, ragged last blocks, no predecessor ----
    // TURN (a compile-time tag): the line's last pair, whose state comes from the forward
    // sweep in registers; its own instance, so that `turn` is dead before the steady loop.
    auto general_iter = [&](int p, auto turn_tag) {
      constexpr bool TURN = decltype(turn_tag)::value;
      const int64_t i0 = (int64_t)(2 * p * K), i1 = i0 + K;
      const IirCoef ce = edge_coefs(blk.job);
      if (p > 0) {
        load_pair(p - 1, na, nb2, false);
        if (p > 1) ck_load(ck, p - 1, nl, Lw, cl, sn);
      }
      const bool head = p == 0;                 // border form at the line start
      const bool tail = i1 + K + 4 > n;         // second block touches the last 4 samples
      const rsrc_t ro = PAIRED ? IFE_OUT_RSRC_RANGE(out + wbase + i0 * st, out_range) : IFE_OUT_RSRC(out + wbase + i0 * st);
      const bool edge = head || (i0 + K + 4 > n);
      CausalState s;
      if (head || TURN) {
        if (head) {
          const double x0 = (double)xa[0];
          s.x1 = s.x2 = s.x3 = x0;
          s.y1 = s.y2 = s.y3 = s.y4 = x0;
        } else {
          s = turn;
        }
        causal_run_park<K>(s, xa, col, ce, i0, n, edge);
      } else {
        // a complete pair behind the line start: from its checkpoint, as in the steady iteration
        s.y1 = sc.y1; s.y2 = sc.y2; s.y3 = sc.y3; s.y4 = sc.y4;
        s.x1 = (double)xa[2]; s.x2 = (double)xa[1]; s.x3 = (double)xa[0];
        col[0] = sc.y3; col[64] = sc.y2; col[128] = sc.y1;
#pragma unroll
        for (int j = 3; j < K; ++j) col[j * 64] = causal_step(s, (double)xa[j], ce);
      }
      if (i1 < n) {  // second block of the pair
        causal_run_park<K>(s, xb, col + K * 64, ce, i1, n, tail);
        anti_run_parked<K>(a, xb, col + K * 64, ce, i1, n, tail);
      }
      anti_run_parked<K>(a, xa, col, ce, i0, n, edge);
      if constexpr (PAIRED) {
        if (is_den) {
#pragma unroll
          for (int j = 0; j < K; ++j) { fx[j * 64] = xa[j]; fx[(K + j) * 64] = xb[j]; }
        }
        lds_workgroup_sync();
        if (!is_den) quotient(i0, i1);
      }
      if (i1 < n) {
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (!tail || i1 + j < n) buf_st_out_f32(ro, voff * 4u, (uint32_t)(K + j) * sst * 4u, xb[j]);
      }
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (!edge || i0 + j < n) buf_st_out_f32(ro, voff * 4u, (uint32_t)j * sst * 4u, xa[j]);
      if constexpr (PAIRED) lds_workgroup_sync();
      rotate();
    };

    const int p_hi = (int)((n - 4) / (2 * K)) - 1;  // largest p with (2p+2)K + 4 <= n
    general_iter(np - 1, std::true_type{});
    int p = np - 2;
    while (p >= 0) {
      if (p >= 2 && p <= p_hi) {
        // The compiler's wait counts inside the loop are only as good as what it knows at the
        // loop's entry (it merges the entry state with the back edge, conservatively): drain
        // once here -- a builtin it accounts for -- so that only the loop's own, unconditional
        // operations are pending inside.  One exposed latency per line.
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        do {
          steady_iter(p);
          --p;
        } while (p >= 2);
      } else {
        general_iter(p, std::false_type{});
        --p;
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// Strided variant with a checkpoint in front of EVERY register block: 16 B/voxel more
// checkpoint traffic than the pair form, but no block is recomputed twice (the pair form
// spends 8 of its 58 double operations per sample on that, and the kernel is bound by
// double-precision issue, not by HBM: with all memory traffic removed it still takes 75 %
// of its time).
// ---------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void iir_strided1_kernel(IirJobs jobs, IirGeom g) {
  const IirBlock blk = iir_block_of(g, blockIdx.x);
  if (!blk.live) return;
  const IirJob &J = jobs.j[blk.job];
  const SrcF32 src{J.in};
  float *__restrict__ out = J.out;
  const IirCoef c = J.c;
  const Checkpoint ck{J.ck_y};
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t Lw =
      uniform64((int64_t)blk.group * blockDim.x + (int64_t)(threadIdx.x & ~63u));
  if (Lw >= g.nlines) return;  // wave-uniform
  const int64_t n = g.n, st = g.sstride, nl = g.nlines;
  int64_t L = Lw + lane;
  const bool live = L < nl;
  if (!live) L = nl - 1;
  const int64_t base = (L % g.inner) + (L / g.inner) * g.outer;
  const int64_t wbase = uniform64(base);
  const uint32_t voff = (uint32_t)(base - wbase);
  const uint32_t sst = (uint32_t)st;
  const int64_t nb = (n + K - 1) / K;

  // ---------------- forward sweep: checkpoint b+1 after block b, b <= nb-2 ----------------
  {
    float xb[K], xn[K];
    CausalState s;
    if (nb > 1) {
      const auto B = src.at(wbase);
#pragma unroll
      for (int j = 0; j < K; ++j) xb[j] = src.ld(B, voff, (uint32_t)j * sst);
    }
    for (int64_t b = 0; b + 1 < nb; ++b) {
      const int64_t i0 = b * K;
      if (b + 2 < nb) {
        const auto B = src.at(wbase + (i0 + K) * st);
#pragma unroll
        for (int j = 0; j < K; ++j) xn[j] = src.ld(B, voff, (uint32_t)j * sst);
      }
      if (b > 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) causal_step(s, (double)xb[j], c);
      } else {
        const double x0 = (double)xb[0];
        s.x1 = s.x2 = s.x3 = x0;
        s.y1 = s.y2 = s.y3 = s.y4 = x0;
#pragma unroll
        for (int j = 0; j < K; ++j) causal_step_edge(s, (double)xb[j], c, j);
      }
      if (live) ck_store(ck, b + 1, nl, Lw, lane, s);
#pragma unroll
      for (int j = 0; j < K; ++j) xb[j] = xn[j];
    }
  }

  // ---------------- backward sweep, one block per iteration ----------------
  {
    float xa[K], na[K];
    float h1 = 0.f, h2 = 0.f, h3 = 0.f, nh1 = 0.f, nh2 = 0.f, nh3 = 0.f;
    AntiState a;
    CausalState sc, sn;
    sc.y1 = sc.y2 = sc.y3 = sc.y4 = 0.0;
    sn = sc;
    auto load_hist = [&](int64_t b, float &q1, float &q2, float &q3) {
      const auto B = src.at(wbase + (b * K - 3) * st);  // b >= 1
      q3 = src.ld(B, voff, 0u);
      q2 = src.ld(B, voff, sst);
      q1 = src.ld(B, voff, 2u * sst);
    };
    {
      const int64_t i0 = (nb - 1) * K;
      const auto B = src.at(wbase + i0 * st);
      const uint32_t lastj = (uint32_t)(n - 1 - i0);
#pragma unroll
      for (int j = 0; j < K; ++j)
        xa[j] = src.ld(B, voff, ((uint32_t)j < lastj ? (uint32_t)j : lastj) * sst);
      if (nb > 1) {
        load_hist(nb - 1, h1, h2, h3);
        ck_load(ck, nb - 1, nl, Lw, live ? lane : 0u, sc);
      }
      const double xN = (double)xa[K - 1];
      a.x1 = a.x2 = a.x3 = a.x4 = xN;
      a.y1 = a.y2 = a.y3 = a.y4 = xN;
    }
    for (int64_t b = nb - 1; b >= 0; --b) {
      const int64_t i0 = b * K;
      if (b > 0) {  // all loads of the iteration come before its stores
        const auto B = src.at(wbase + (i0 - K) * st);
#pragma unroll
        for (int j = 0; j < K; ++j) na[j] = src.ld(B, voff, (uint32_t)j * sst);
        if (b > 1) {
          load_hist(b - 1, nh1, nh2, nh3);
          ck_load(ck, b - 1, nl, Lw, live ? lane : 0u, sn);
        }
      }
      CausalState s;
      if (b > 0) {
        s.y1 = sc.y1; s.y2 = sc.y2; s.y3 = sc.y3; s.y4 = sc.y4;
        s.x1 = (double)h1; s.x2 = (double)h2; s.x3 = (double)h3;
      } else {
        const double x0 = (double)xa[0];
        s.x1 = s.x2 = s.x3 = x0;
        s.y1 = s.y2 = s.y3 = s.y4 = x0;
      }
      const bool edge = (b == 0) || (i0 + K + 4 > n);
      double cz[K];
      causal_run<K, true>(s, xa, cz, c, i0, n, edge);
      anti_run<K>(a, xa, cz, c, i0, n, edge);
      if (live) {
        const rsrc_t ro = IFE_OUT_RSRC(out + wbase + i0 * st);
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (!edge || i0 + j < n) buf_st_out_f32(ro, voff * 4u, (uint32_t)j * sst * 4u, xa[j]);
      }
#pragma unroll
      for (int j = 0; j < K; ++j) xa[j] = na[j];
      h1 = nh1; h2 = nh2; h3 = nh3;
      sc.y1 = sn.y1; sc.y2 = sn.y2; sc.y3 = sn.y3; sc.y4 = sn.y4;
    }
  }
}

// ---------------------------------------------------------------------------------
// Shared causal sweep of the first axis pass (Z), one launch in front of the backward-only
// form of iir_strided_kernel.  All scales of a group filter the SAME two fields, so the causal
// recursions of one line run side by side in one lane: every sample is loaded and converted
// once, from the image and the mask themselves, and the prepass and its round trip through
// memory go away.  A wave owns 64 x-adjacent lines of ONE field (workgroups are numbered
// field-fastest through iir_block_of with njobs = fields, so the two fields of a line group
// meet in one XCD's L2 for the mask): NS chains per lane, the x history shared between them,
// and the denominator waves never read the image.  Per register block of K samples it
//   * loads TI image and TM mask and forms t = float(image) * float(mask), c = float(mask)
//     exactly as prep_kernel_* does (no mask: t = float(image), no multiply),
//   * stores its field's value as the float source of the backward sweeps -- for EVERY sample
//     of the line, the last (ragged) pair included, which is not recursed over,
//   * advances the NS recursions; three samples into every pair 1 .. np-2 their y1..y4 go to
//     the jobs' checkpoint areas (layout of ck_store), and after pair np-2 -- the state in
//     front of the last pair -- to the slot of pair np-1, which no pair checkpoint uses,
//   * where a job copies constant lines, compares every swept sample with the first and leaves
//     the field's per-line record (IirJob::line_rec).
// Every memory operation of the sweep is unconditional: a descriptor ends with the volume
// (rows past the line end load zeros and drop their stores), and a field that is not read or
// not written has an empty one.  A lane past the last line repeats the last line.
// ---------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ uint32_t buf_ld_raw(rsrc_t r, uint32_t voff, uint32_t soff);
template <>
__device__ __forceinline__ uint32_t buf_ld_raw<float>(rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}
template <>
__device__ __forceinline__ uint32_t buf_ld_raw<int16_t>(rsrc_t r, uint32_t voff, uint32_t soff) {
  return (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0);
}
template <>
__device__ __forceinline__ uint32_t buf_ld_raw<uint16_t>(rsrc_t r, uint32_t voff, uint32_t soff) {
  return (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0);
}
template <>
__device__ __forceinline__ uint32_t buf_ld_raw<uint8_t>(rsrc_t r, uint32_t voff, uint32_t soff) {
  return (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(r, voff, soff, 0);
}
template <typename T>
__device__ __forceinline__ float raw_as_f32(uint32_t r) {
  if constexpr (std::is_same<T, float>::value) return __builtin_bit_cast(float, r);
  else if constexpr (std::is_same<T, int16_t>::value) return (float)(int16_t)(uint16_t)r;
  else return (float)r;
}
struct SweepY {
  double y1, y2, y3, y4;
};
// causal_step with the x history outside the state (it is the same for every scale)
template <typename C>
__device__ __forceinline__ void sweep_step(SweepY &s, double x1, double x2, double x3, double xin, const C &c) {
  const double a = IFE_MADD(x3, c.N3, IFE_MADD(x2, c.N2, IFE_MADD(x1, c.N1, xin * c.N0)));
  const double t = IFE_MADD(s.y4, c.D4, IFE_MADD(s.y3, c.D3, IFE_MADD(s.y2, c.D2, s.y1 * c.D1)));
  const double y = a - t;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
}
struct SweepCoef {
  double N0, N1, N2, N3, D1, D2, D3, D4;
};
template <int K, int NS, typename TI, typename TM>
__global__ __launch_bounds__(256, K <= 12 ? 4 : 3) void iir_sweep_z_kernel(IirJobs jobs, IirGeom g, ZSweepArgs a) {
  const IirBlock blk = iir_block_of(g, blockIdx.x);  // g.njobs = fields: blk.job is the field
  if (!blk.live) return;
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t Lw = uniform64((int64_t)blk.group * blockDim.x + (int64_t)(threadIdx.x & ~63u));
  if (Lw >= g.nlines) return;  // wave-uniform
  const uint32_t f = blk.job, nf = (uint32_t)a.nf;
  const bool is_den = f != 0u;
  const bool has_mask = a.msk != nullptr;
  // Z axis: line L starts at element L, samples are nl elements apart
  const int64_t n = g.n, nl = g.nlines;
  int64_t L = Lw + lane;
  if (L >= nl) L = nl - 1;  // a lane past the last line repeats the last line
  const uint32_t cl = (uint32_t)(L - Lw);
  const uint32_t sst = (uint32_t)nl;  // 2K*nl*4 < 2^31 is checked on the host
  const int nb = (int)((n + K - 1) / K);
  const int np = (nb + 1) / 2;
  const int nfp = np - 1;  // complete pairs in front of the last one: the swept part of the line
  float *const dst = reinterpret_cast<float *>(uniform64(reinterpret_cast<int64_t>(is_den ? a.cf : a.tc)));
  // all ones / zero, as integers (mask_lt's comment): which streams this wave really moves
  const uint32_t rd_img = is_den ? 0u : 0xffffffffu;
  const uint32_t rd_msk = has_mask ? 0xffffffffu : 0u;
  const uint32_t wr_src = a.write_src != 0 ? 0xffffffffu : 0u;

  SweepCoef c[NS];
  double *cky[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const IirJob &J = jobs.j[(uint32_t)k * nf + f];
    c[k] = SweepCoef{J.c.N0, J.c.N1, J.c.N2, J.c.N3, J.c.D1, J.c.D2, J.c.D3, J.c.D4};
    cky[k] = J.ck_y;
  }

  uint32_t ri[K], rm[K];  // the next register block of raw image and mask, in flight
  float v[K];
  SweepY s[NS];
  double x1 = 0.0, x2 = 0.0, x3 = 0.0;
  bool cst = true;
  uint32_t ref = 0u;

  // Descriptors are rebuilt for every G rows (three scalar offsets per element size instead of
  // K - 1).  Their range, in 32-bit scalar integer arithmetic: the elements from lane 0's
  // sample in row `row` to the end of the volume, of at most 2K rows (more is never reached
  // from one base, and 2K * nl * 4 < 2^31), nothing from the line's end on.
  constexpr int G = K % 4 == 0 ? 4 : 2;
  const int ni = (int)n;
  const uint32_t nlu = (uint32_t)nl, lwu = (uint32_t)Lw;  // Lw < nl < 2^26
  auto range_of = [&](int row, uint32_t esize) -> uint32_t {
    int rows = ni - row;
    rows = rows < 0 ? 0 : rows;
    rows = rows > 2 * K ? 2 * K : rows;
    const uint32_t one = rows > 0 ? 1u : 0u;  // s_min: no lane mask
    return ((uint32_t)rows * nlu - one * lwu) * esize;
  };
  auto load_blk = [&](int b, uint32_t (&ri)[K], uint32_t (&rm)[K]) {
    __builtin_amdgcn_sched_barrier(0);  // behind the conversions that free these registers
#pragma unroll
    for (int q = 0; q < K; q += G) {
      const int row = b * K + q;
      const int64_t e0 = Lw + (int64_t)row * nl;
      const rsrc_t dI = make_rsrc_range(static_cast<const TI *>(a.img) + e0, range_of(row, sizeof(TI)) & rd_img);
#pragma unroll
      for (int j = 0; j < G; ++j)
        ri[q + j] = buf_ld_raw<TI>(dI, cl * (uint32_t)sizeof(TI), (uint32_t)j * sst * (uint32_t)sizeof(TI));
    }
#pragma unroll
    for (int q = 0; q < K; q += G) {
      const int row = b * K + q;
      const int64_t e0 = Lw + (int64_t)row * nl;
      const rsrc_t dM = make_rsrc_range(static_cast<const TM *>(has_mask ? a.msk : a.img) + e0,
                                        range_of(row, sizeof(TM)) & rd_msk);
#pragma unroll
      for (int j = 0; j < G; ++j)
        rm[q + j] = buf_ld_raw<TM>(dM, cl * (uint32_t)sizeof(TM), (uint32_t)j * sst * (uint32_t)sizeof(TM));
    }
  };
  // raw -> this wave's field, and its source rows for the backward sweeps
  auto take_blk = [&](int b, const uint32_t (&ri)[K], const uint32_t (&rm)[K]) {
    // (scheduling fence: left alone, the conversions move up into the recursion in front of
    // them, and with them the wait for loads that were issued a moment ago)
    __builtin_amdgcn_sched_barrier(0);
    if (is_den) {  // uniform branches over arithmetic only
#pragma unroll
      for (int j = 0; j < K; ++j) v[j] = raw_as_f32<TM>(rm[j]);
    } else if (has_mask) {
#pragma unroll
      for (int j = 0; j < K; ++j) v[j] = raw_as_f32<TI>(ri[j]) * raw_as_f32<TM>(rm[j]);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) v[j] = raw_as_f32<TI>(ri[j]);
    }
#pragma unroll
    for (int q = 0; q < K; q += G) {
      const int row = b * K + q;
      const rsrc_t dO = make_rsrc_range(dst + Lw + (int64_t)row * nl, range_of(row, 4u) & wr_src);
#pragma unroll
      for (int j = 0; j < G; ++j) buf_st_f32(dO, cl * 4u, (uint32_t)j * sst * 4u, v[q + j]);
    }
  };
  auto track = [&]() {
    if (a.track) {  // uniform
#pragma unroll
      for (int j = 0; j < K; ++j) cst = cst && __builtin_bit_cast(uint32_t, v[j]) == ref;
    }
  };
  auto run = [&](int j0, int j1) {
#pragma unroll
    for (int j = j0; j < j1; ++j) {
      const double xin = (double)v[j];
#pragma unroll
      for (int k = 0; k < NS; ++k) sweep_step(s[k], x1, x2, x3, xin, c[k]);
      x3 = x2; x2 = x1; x1 = xin;
    }
  };
  auto store_state = [&](int slot) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      // (made scalar by hand: a base the compiler has parked in a vector register turns every
      // store into a loop over "distinct" descriptors, and all wait counts around it to zero)
      double *const base = reinterpret_cast<double *>(uniform64(reinterpret_cast<int64_t>(cky[k])));
      const rsrc_t ry = IFE_CK_RSRC(base + ((int64_t)slot * 4) * nl + Lw);
      const uint32_t sy = (uint32_t)nl * 8u;
      ck_st_f64(ry, cl * 8u, 0u, s[k].y1);
      ck_st_f64(ry, cl * 8u, sy, s[k].y2);
      ck_st_f64(ry, cl * 8u, 2u * sy, s[k].y3);
      ck_st_f64(ry, cl * 8u, 3u * sy, s[k].y4);
    }
  };

  // One block ahead: a block is converted (take_blk) and the next one requested into the same
  // registers before the recursion runs over it -- 45 double operations per sample and scale
  // group of latency cover, at four waves per SIMD where K <= 12.
  load_blk(0, ri, rm);
  if (nfp > 0) {
    // pair 0: border form on the first block (causal_step_edge, each scale with its own
    // border coefficients), then the interior form
    take_blk(0, ri, rm);
    load_blk(1, ri, rm);
    ref = __builtin_bit_cast(uint32_t, v[0]);
    {
      const double e0 = (double)v[0];
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const IirCoef ce = edge_coefs((uint32_t)k * nf + f);
        CausalState e;
        e.x1 = e.x2 = e.x3 = e0;
        e.y1 = e.y2 = e.y3 = e.y4 = e0;
#pragma unroll
        for (int j = 0; j < K; ++j) causal_step_edge(e, (double)v[j], ce, j);
        s[k] = SweepY{e.y1, e.y2, e.y3, e.y4};
      }
      x1 = (double)v[K - 1]; x2 = (double)v[K - 2]; x3 = (double)v[K - 3];
    }
    track();
    take_blk(1, ri, rm);
    load_blk(2, ri, rm);
    run(0, K);
    track();
    for (int p = 1; p < nfp; ++p) {
      take_blk(2 * p, ri, rm);
      load_blk(2 * p + 1, ri, rm);
      run(0, 3);
      store_state(p);  // three samples into the pair (ck_store)
      run(3, K);
      track();
      take_blk(2 * p + 1, ri, rm);
      load_blk(2 * p + 2, ri, rm);
      run(0, K);
      track();
    }
    store_state(np - 1);  // the state in front of the last pair
    if (a.track) a.rec[(int64_t)f * nl + L] = cst ? ref : ZSWEEP_NOT_CONST;
  }
  // the last pair: sources only (its second block may lie past the line end: nothing moves)
  take_blk(2 * nfp, ri, rm);
  load_blk(2 * nfp + 1, ri, rm);
  take_blk(2 * nfp + 1, ri, rm);
}

// =================================================================================
// contiguous axis (X): 64 lines x 2K samples staged through LDS per wave
// =================================================================================
// A tile is two register blocks wide (2K = 32 samples = 128 B per line), so every global
// access of a line is one whole 128-B cache line; with K-wide tiles each line was
// fetched twice (PMC: 46 % over-fetch on the X pass).
template <int W>
struct XTile {
  static constexpr int PITCH = W + 4;  // floats; keeps rows 16-B aligned, conflict-free b128 reads
  static constexpr int FLOATS = 64 * PITCH;
};

// A wave's DS instructions execute in order, so a tile written and then read by the
// same wave needs no barrier: only the compiler must be kept from moving LDS
// accesses across this point (the "memory" clobber), and global traffic in flight
// is left alone (no vmcnt wait, unlike a workgroup-scope fence).
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Fill the wave's LDS tile with samples [i0, i0+W) of its 64 lines.  Samples past the
// line end repeat x[n-1].  `rows` points at sample 0 of the wave's first line (uniform).
template <int W, int AUX = 0>
__device__ __forceinline__ void xtile_fill(const float *rows, float *tile, uint32_t lane,
                                           int64_t nrows, int64_t pitch, int64_t i0, int64_t n,
                                           bool vec_ok) {
  constexpr int P = XTile<W>::PITCH;
  constexpr int V = W / 4;     // float4 per line
  constexpr int LPI = 64 / V;  // lines covered per wave instruction
  if (vec_ok && i0 + W <= n) {
    const rsrc_t r4 = make_rsrc(rows + i0);
    u32x4 v[V];
#pragma unroll
    for (int r = 0; r < V; ++r) {
      uint32_t row = (lane / V) + r * LPI;
      if ((int64_t)row >= nrows) row = (uint32_t)(nrows - 1);
      const uint32_t off = (row * (uint32_t)pitch + 4u * (lane % V)) * 4u;
      v[r] = __builtin_amdgcn_raw_buffer_load_b128(r4, off, 0u, AUX);
    }
#pragma unroll
    for (int r = 0; r < V; ++r)
      *reinterpret_cast<u32x4 *>(tile + ((lane / V) + r * LPI) * P + 4 * (lane % V)) = v[r];
  } else {  // unaligned or ragged tile: rolled loop (rare path, keep its footprint small)
#pragma clang loop unroll(disable)
    for (int e = 0; e < W; ++e) {
      const uint32_t idx = e * 64 + lane;
      uint32_t row = idx / W;
      const uint32_t col = idx % W;
      const uint32_t trow = row;
      if ((int64_t)row >= nrows) row = (uint32_t)(nrows - 1);
      int64_t i = i0 + col;
      if (i >= n) i = n - 1;
      tile[trow * P + col] = rows[(int64_t)row * pitch + i];
    }
  }
  wave_lds_sync();
}

// Register block h (K samples) of the lane's own line, out of / back into the tile.
template <int W, int K>
__device__ __forceinline__ void xtile_get(const float *tile, uint32_t lane, int h, float (&xb)[K]) {
  constexpr int P = XTile<W>::PITCH;
#pragma unroll
  for (int q = 0; q < K / 4; ++q) {
    const float4 t = *reinterpret_cast<const float4 *>(tile + lane * P + h * K + 4 * q);
    xb[4 * q + 0] = t.x; xb[4 * q + 1] = t.y; xb[4 * q + 2] = t.z; xb[4 * q + 3] = t.w;
  }
}
template <int W, int K>
__device__ __forceinline__ void xtile_put(float *tile, uint32_t lane, int h, const float (&xb)[K]) {
  constexpr int P = XTile<W>::PITCH;
#pragma unroll
  for (int q = 0; q < K / 4; ++q)
    *reinterpret_cast<float4 *>(tile + lane * P + h * K + 4 * q) =
        make_float4(xb[4 * q + 0], xb[4 * q + 1], xb[4 * q + 2], xb[4 * q + 3]);
}

// Write the tile back to samples [i0, i0+W) of the lines (valid samples only).
template <int W>
__device__ __forceinline__ void xtile_drain(float *rows, float *tile, uint32_t lane,
                                            int64_t nrows, int64_t pitch, int64_t i0, int64_t n,
                                            bool vec_ok) {
  constexpr int P = XTile<W>::PITCH;
  constexpr int V = W / 4;
  constexpr int LPI = 64 / V;
  wave_lds_sync();
  if (vec_ok && i0 + W <= n) {
    const rsrc_t r4 = make_rsrc(rows + i0);
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const uint32_t row = (lane / V) + r * LPI;
      const u32x4 v = *reinterpret_cast<const u32x4 *>(tile + row * P + 4 * (lane % V));
      const uint32_t off = (row * (uint32_t)pitch + 4u * (lane % V)) * 4u;
      if ((int64_t)row < nrows) __builtin_amdgcn_raw_buffer_store_b128(v, r4, off, 0u, IFE_OUT_AUX);
    }
  } else {
#pragma clang loop unroll(disable)
    for (int e = 0; e < W; ++e) {
      const uint32_t idx = e * 64 + lane;
      const uint32_t row = idx / W, col = idx % W;
      const int64_t i = i0 + col;
      if ((int64_t)row < nrows && i < n) rows[(int64_t)row * pitch + i] = tile[row * P + col];
    }
  }
  wave_lds_sync();
}

template <int K>
__global__ __launch_bounds__(256, 2) void iir_contig_kernel(IirJobs jobs, IirGeom g) {
  const IirBlock blk = iir_block_of(g, blockIdx.x);
  if (!blk.live) return;
  const IirJob &J = jobs.j[blk.job];
  const float *__restrict__ in = J.in;
  float *__restrict__ out = J.out;
  const IirCoefMain c = main_coefs(J.c);  // interior recursion; border tiles read edge_coefs(blk.job)
  const Checkpoint ck{J.ck_y};
  constexpr int W = 2 * K;  // tile width: two register blocks
  constexpr int P = XTile<W>::PITCH;
  constexpr int V = W / 4;     // 16-byte pieces per line and tile
  constexpr int LPI = 64 / V;  // lines one wave instruction covers
  __shared__ __attribute__((aligned(16))) float lds[4 * XTile<W>::FLOATS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *tile = lds + wave * XTile<W>::FLOATS;
#if IFE_IIR_LDS_CZ
  __shared__ double park[4][K][64];
  double *col = &park[wave][0][lane];
#else
#error "the contiguous-axis kernel parks the causal values of a tile's first block in LDS"
#endif
  const int64_t line0 = uniform64(((int64_t)blk.group * 4 + wave) * 64);
  if (line0 >= g.nlines) return;
  const int64_t n = g.n, nl = g.nlines, pitch = g.outer;
  const int64_t nrows = nl - line0 < 64 ? nl - line0 : 64;  // live lines of this wave
  const int nt = (int)((n + W - 1) / W);
  // 16-B accesses need aligned rows; the per-lane byte offset must fit 32 bits
  const bool vec_ok = (pitch % 4 == 0) && ((reinterpret_cast<uintptr_t>(in) & 15) == 0) &&
                      ((reinterpret_cast<uintptr_t>(out) & 15) == 0) &&
                      (pitch * 64 * 4 < (int64_t)0x7fffffff);
  const bool live = (int64_t)lane < nrows;
  int64_t in_line0 = line0;
  if (g.in_w > 1) {
    const int64_t gi = line0 / g.in_group, within = line0 % g.in_group;  // gi = z*in_w + h
    in_line0 = ((gi % g.in_w) * g.in_nz + gi / g.in_w) * g.in_group + within;
  }
  const float *rows_in = in + in_line0 * pitch;
  float *rows_out = out + line0 * pitch;

  // Pipelined form (the common case: aligned rows, all 64 lines of the wave live): the next
  // tile travels from memory into registers while the current one is computed, the drained
  // tile's stores stay in flight behind it, and -- as in the strided kernel -- the steady loops
  // hold no conditional memory operation, so the compiler's waits are exact.  Everything
  // else (ragged rows, a partial last wave, the tiles at the ends of the line) takes the
  // plain form: fill, wait, compute, drain.
  const bool piped = vec_ok && nrows == 64;  // wave-uniform
  const uint32_t prow = lane / V, pchunk = lane % V;  // this lane's piece of a wave instruction
  const uint32_t voff_g = (prow * (uint32_t)pitch + 4u * pchunk) * 4u;
  const uint32_t sp = (uint32_t)LPI * (uint32_t)pitch * 4u;  // bytes between successive instructions' lines
  float *const tpiece = tile + prow * P + 4 * pchunk;
  u32x4 pf[V];  // the tile in flight
  auto issue_fill = [&](int t, uint32_t range) {
    const rsrc_t r4 = make_rsrc_range(rows_in + (int64_t)t * W, range);
#pragma unroll
    for (int r = 0; r < V; ++r) pf[r] = __builtin_amdgcn_raw_buffer_load_b128(r4, voff_g, (uint32_t)r * sp, 0);
  };
  auto commit_fill = [&]() {
#pragma unroll
    for (int r = 0; r < V; ++r) *reinterpret_cast<u32x4 *>(tpiece + r * LPI * P) = pf[r];
    wave_lds_sync();
  };
  auto drain_piped = [&](int t) {
    wave_lds_sync();
    const rsrc_t r4 = make_rsrc(rows_out + (int64_t)t * W);
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const u32x4 v = *reinterpret_cast<const u32x4 *>(tpiece + r * LPI * P);
      __builtin_amdgcn_raw_buffer_store_b128(v, r4, voff_g, (uint32_t)r * sp, IFE_OUT_AUX);
    }
    wave_lds_sync();
  };

  float xb[K];

  // ---------------- forward sweep: a checkpoint for every tile 1 .. nt-2 ----------------
  // As in the strided kernel the checkpoint of a tile is taken three samples into it (its x
  // history is then the tile's own first three samples, and nothing but the four y values is
  // kept), and the state in front of the last tile goes to the backward sweep in registers.
  bool fwd_const = true;  // constant lines, as in the strided kernel
  float fwd_ref = 0.0f;
  CausalState turn;
  turn.x1 = turn.x2 = turn.x3 = 0.0;
  turn.y1 = turn.y2 = turn.y3 = turn.y4 = 0.0;
  {
    CausalState s;
    // both blocks of tile t from LDS through the causal recursion (tile 0: border form)
    auto fwd_tile = [&](int t) {
#pragma clang loop unroll(disable)
      for (int h = 0; h < 2; ++h) {
        xtile_get<W, K>(tile, lane, h, xb);
        if (t > 0 || h > 0) {
#pragma unroll
          for (int j = 0; j < 3; ++j) causal_step(s, (double)xb[j], c);
          if (t > 0 && h == 0 && live) ck_store(ck, t, nl, line0, lane, s);
#pragma unroll
          for (int j = 3; j < K; ++j) causal_step(s, (double)xb[j], c);
        } else {
          const IirCoef ce = edge_coefs(blk.job);
          const double x0 = (double)xb[0];
          fwd_ref = xb[0];
          s.x1 = s.x2 = s.x3 = x0;
          s.y1 = s.y2 = s.y3 = s.y4 = x0;
#pragma unroll
          for (int j = 0; j < K; ++j) causal_step_edge(s, (double)xb[j], ce, j);
        }
        if (J.const_lines) {
#pragma unroll
          for (int j = 0; j < K; ++j) fwd_const = fwd_const && same_bits(xb[j], fwd_ref);
        }
      }
    };
    const int ntf = nt - 1;  // tiles 0 .. ntf-1, all complete
    if (piped) {
      if (ntf > 0) {
        issue_fill(0, 0xffffffffu);
        commit_fill();
        issue_fill(1, mask_lt(1, ntf));
        fwd_tile(0);
        wave_lds_sync();
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): see the strided kernel's steady loop
        for (int t = 1; t < ntf; ++t) {
          commit_fill();
          issue_fill(t + 1, mask_lt(t + 1, ntf));  // beyond the sweep: dropped
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            xtile_get<W, K>(tile, lane, h, xb);
#pragma unroll
            for (int j = 0; j < 3; ++j) causal_step(s, (double)xb[j], c);
            if (h == 0) ck_store(ck, t, nl, line0, lane, s);
#pragma unroll
            for (int j = 3; j < K; ++j) causal_step(s, (double)xb[j], c);
            if (J.const_lines) {
#pragma unroll
              for (int j = 0; j < K; ++j) fwd_const = fwd_const && same_bits(xb[j], fwd_ref);
            }
          }
          wave_lds_sync();  // reads of this tile are done before the next commit overwrites it
        }
      }
    } else {
      for (int t = 0; t < ntf; ++t) {
        xtile_fill<W>(rows_in, tile, lane, nrows, pitch, (int64_t)t * W, n, vec_ok);
        fwd_tile(t);
        wave_lds_sync();  // reads of this tile are done before the next fill overwrites it
      }
    }
    if (ntf > 0) turn = s;
  }

  // ---------------- backward sweep, one tile (pair of blocks) per iteration ----------------
  {
    AntiState a;
    bool done = false;  // the constant-line shortcut has answered the whole line
    // plain form of one tile: fill, wait, compute with every border rule, drain
    // TURN (a compile-time tag): the line's last tile, which starts from `turn`
    auto plain_tile = [&](int t, auto turn_tag) {
      constexpr bool TURN = decltype(turn_tag)::value;
      const int64_t i0 = (int64_t)t * W, i1 = i0 + K;
      const IirCoef ce = edge_coefs(blk.job);
      xtile_fill<W, IFE_IN2_AUX>(rows_in, tile, lane, nrows, pitch, i0, n, vec_ok);
      if constexpr (TURN) {
        // x[n-1]: the clamped fill makes every slot past the line end hold it
        const double xN = (double)tile[lane * P + W - 1];
        a.x1 = a.x2 = a.x3 = a.x4 = xN;
        a.y1 = a.y2 = a.y3 = a.y4 = xN;
        if (J.const_lines) {  // uniform: are all 64 lines 0 (or 1 where allowed) throughout?
          float xa0[K], xb0[K];
          xtile_get<W, K>(tile, lane, 0, xa0);
          xtile_get<W, K>(tile, lane, 1, xb0);
          const float first = xa0[0];
          bool cst = nt == 1 || (fwd_const && same_bits(fwd_ref, first));
#pragma unroll
          for (int j = 0; j < K; ++j) cst = cst && same_bits(xa0[j], first) && same_bits(xb0[j], first);
          float resp;
          cst = const_line_response(__builtin_bit_cast(uint32_t, first), J.const_lines, resp) && cst;
          if (__builtin_amdgcn_ballot_w64(!cst && live) == 0) {
            // every row that is stored holds its constant; where the answer differs from the
            // input (a line of -0 answered with +0) the row is rewritten first
            if (__builtin_amdgcn_ballot_w64(live && !same_bits(resp, first)) != 0) {
              wave_lds_sync();
              if (live && !same_bits(resp, first)) {
#pragma unroll
                for (int j = 0; j < W; ++j) tile[lane * P + j] = resp;
              }
              wave_lds_sync();
            }
            // drain the tile over the line
            for (int tt = nt - 1; tt >= 0; --tt)
              xtile_drain<W>(rows_out, tile, lane, nrows, pitch, (int64_t)tt * W, n, vec_ok);
            done = true;
            return;
          }
        }
      }
      CausalState s0;
      float xa[K];
      xtile_get<W, K>(tile, lane, 0, xa);
      const bool head = t == 0;
      if (head) {
        const double x0 = (double)xa[0];
        s0.x1 = s0.x2 = s0.x3 = x0;
        s0.y1 = s0.y2 = s0.y3 = s0.y4 = x0;
      } else if constexpr (TURN) {
        s0 = turn;
      } else {
        ck_load(ck, t, nl, line0, live ? lane : 0u, s0);
        s0.x1 = (double)xa[2]; s0.x2 = (double)xa[1]; s0.x3 = (double)xa[0];
      }
      double cz[K];
      const bool edge = head || (i0 + K + 4 > n);
      if (i1 < n) {
        const bool tail = i1 + K + 4 > n;
        CausalState s = s0;
        if (head || TURN) {
          causal_run_park<K>(s, xa, col, ce, i0, n, head);
        } else {  // a complete tile behind the line start: its checkpoint is its first three causal values
          col[0] = s0.y3; col[64] = s0.y2; col[128] = s0.y1;
#pragma unroll
          for (int j = 3; j < K; ++j) col[j * 64] = causal_step(s, (double)xa[j], ce);
        }
        xtile_get<W, K>(tile, lane, 1, xb);
        causal_run<K, true>(s, xb, cz, ce, i1, n, tail);
        anti_run<K>(a, xb, cz, ce, i1, n, tail);
        xtile_put<W, K>(tile, lane, 1, xb);
        __builtin_amdgcn_sched_barrier(0);
        xtile_get<W, K>(tile, lane, 0, xa);
        anti_run_parked<K>(a, xa, col, ce, i0, n, edge);
      } else {
        CausalState s = s0;
        causal_run<K, true>(s, xa, cz, ce, i0, n, edge);
        anti_run<K>(a, xa, cz, ce, i0, n, edge);
      }
      xtile_put<W, K>(tile, lane, 0, xa);
      xtile_drain<W>(rows_out, tile, lane, nrows, pitch, i0, n, vec_ok);
    };

    // checkpoint of the tile in flight (steady tiles)
    double ny1 = 0.0, ny2 = 0.0, ny3 = 0.0, ny4 = 0.0;
    auto issue_ck = [&](int tt, uint32_t range) {
      const rsrc_t ry = make_rsrc_range(ck.y + ((int64_t)tt * 4) * nl + line0, range);
      const uint32_t sy = (uint32_t)nl * 8u;
      ny1 = ck_ld_f64(ry, lane * 8u, 0u);
      ny2 = ck_ld_f64(ry, lane * 8u, sy);
      ny3 = ck_ld_f64(ry, lane * 8u, 2u * sy);
      ny4 = ck_ld_f64(ry, lane * 8u, 3u * sy);
    };
    // steady tiles: away from both ends of the line, (t+1)W + 4 <= n and t >= 1
    const int t_hi = piped ? (int)((n - 4) / W) - 1 : -1;
    plain_tile(nt - 1, std::true_type{});
    int t = nt - 2;
    while (t >= 0 && !done) {
      if (t >= 1 && t <= t_hi) {
        // ---- tile t-1 and its checkpoint travel while tile t is computed ----
        issue_fill(t, 0xffffffffu);
        issue_ck(t, 0xffffffffu);
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): only the loop's own operations are pending inside
        do {
          commit_fill();
          CausalState s;
          s.y1 = ny1; s.y2 = ny2; s.y3 = ny3; s.y4 = ny4;
          col[0] = ny3; col[64] = ny2; col[128] = ny1;  // the tile's first three causal values
          issue_fill(t - 1, 0xffffffffu);
          issue_ck(t - 1, mask_lt(1, t));  // tile 0 starts the line: no checkpoint
          float xa[K];
          double cz[K];
          xtile_get<W, K>(tile, lane, 0, xa);
          s.x1 = (double)xa[2]; s.x2 = (double)xa[1]; s.x3 = (double)xa[0];
#pragma unroll
          for (int j = 3; j < K; ++j) col[j * 64] = causal_step(s, (double)xa[j], c);
          xtile_get<W, K>(tile, lane, 1, xb);
#pragma unroll
          for (int j = 0; j < K; ++j) cz[j] = causal_step(s, (double)xb[j], c);
#pragma unroll
          for (int j = K - 1; j >= 0; --j) xb[j] = (float)(cz[j] + anti_step(a, (double)xb[j], c));
          xtile_put<W, K>(tile, lane, 1, xb);
          __builtin_amdgcn_sched_barrier(0);
          xtile_get<W, K>(tile, lane, 0, xa);
#pragma unroll
          for (int j = K - 1; j >= 0; --j) xa[j] = (float)(col[j * 64] + anti_step(a, (double)xa[j], c));
          xtile_put<W, K>(tile, lane, 0, xa);
          drain_piped(t);
          --t;
        } while (t >= 1);
      } else {
        plain_tile(t, std::false_type{});
        --t;
      }
    }
  }
}

// =================================================================================
// Z pass of a Z-slab: causal sweep, anticausal sweep, combine (iir_types.hpp "ZSlabJob")
// =================================================================================
// Three launches instead of the single-device kernel's one, because the two recursions
// arrive from opposite neighbours at different times: each sweep is one recursion step per
// sample and sits on the critical chain across the devices (state in -> sweep -> state
// out), the combine (two steps per sample, pairs independent of each other) is local.
// Border rule: a slab with a neighbour never uses ITK's border coefficients on that side;
// `ioff` / `nedge` shift the indices the border tests see so that they never fire.
struct SlabLine {
  uint32_t lane;
  int64_t Lw;
  bool live;
  uint32_t voff;  // lane's element offset from the wave's first line
};
__device__ __forceinline__ bool slab_line(const ZSlabGeom &g, uint32_t group, SlabLine &l) {
  l.lane = threadIdx.x & 63u;
  l.Lw = uniform64((int64_t)group * blockDim.x + (int64_t)(threadIdx.x & ~63u));
  if (l.Lw >= g.nlines) return false;  // wave-uniform
  const int64_t L = l.Lw + l.lane;
  l.live = L < g.nlines;
  l.voff = l.live ? l.lane : (uint32_t)(g.nlines - 1 - l.Lw);  // compute on a valid line, never store
  return true;
}
__device__ __forceinline__ IirBlock slab_block_of(const ZSlabGeom &g, uint32_t lin) {
  IirGeom t;
  t.njobs = g.njobs;
  t.ngroups = g.ngroups;
  return iir_block_of(t, lin);
}
// state records and checkpoints: [4][stride] doubles (the x history of either is re-read from
// the samples, those of a neighbour included: iir_types.hpp "ZSlabJob")
__device__ __forceinline__ void y4_store(double *y, int64_t stride, int64_t Lw, uint32_t voff, double y1,
                                         double y2, double y3, double y4) {
  const rsrc_t ry = IFE_CK_RSRC(y + Lw);
  const uint32_t sy = (uint32_t)stride * 8u;
  buf_st_f64(ry, voff * 8u, 0u, y1);
  buf_st_f64(ry, voff * 8u, sy, y2);
  buf_st_f64(ry, voff * 8u, 2u * sy, y3);
  buf_st_f64(ry, voff * 8u, 3u * sy, y4);
}
__device__ __forceinline__ void y4_load(const double *y, int64_t stride, int64_t Lw, uint32_t voff,
                                        double &y1, double &y2, double &y3, double &y4) {
  const rsrc_t ry = IFE_CK_RSRC(y + Lw);
  const uint32_t sy = (uint32_t)stride * 8u;
  y1 = buf_ld_f64(ry, voff * 8u, 0u);
  y2 = buf_ld_f64(ry, voff * 8u, sy);
  y3 = buf_ld_f64(ry, voff * 8u, 2u * sy);
  y4 = buf_ld_f64(ry, voff * 8u, 3u * sy);
}
// x[first], x[first + 1], ... of the lane's line, `first` relative to the slab's plane 0 and
// possibly outside it (a neighbour's planes)
template <int N>
__device__ __forceinline__ void slab_load_planes(const float *in, const ZSlabGeom &g, int64_t Lw,
                                                 uint32_t voff, int64_t first, float (&v)[N]) {
  const rsrc_t r = make_rsrc(in + Lw + first * g.sstride);
  const uint32_t sst = (uint32_t)g.sstride;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = buf_ld_f32(r, voff * 4u, (uint32_t)k * sst * 4u);
}
// K samples starting at plane i0 of the lane's line; planes past the slab repeat the last one
template <int K>
__device__ __forceinline__ void slab_load_block(const float *in, const ZSlabGeom &g, int64_t Lw,
                                                uint32_t voff, int64_t i0, float (&x)[K]) {
  const rsrc_t r = IFE_IN_RSRC(in + Lw + i0 * g.sstride);
  const uint32_t sst = (uint32_t)g.sstride;
  if (i0 + K <= g.n) {
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = buf_ld_f32(r, voff * 4u, (uint32_t)j * sst * 4u);
  } else {
    const uint32_t lastj = (uint32_t)(g.n - 1 - i0);
#pragma unroll
    for (int j = 0; j < K; ++j)
      x[j] = buf_ld_f32(r, voff * 4u, ((uint32_t)j < lastj ? (uint32_t)j : lastj) * sst * 4u);
  }
}

// ---- causal sweep: state in (or ITK's start of line), checkpoints, state out ----------
template <int K>
__global__ __launch_bounds__(256) void zslab_causal_kernel(ZSlabJobs jobs, ZSlabGeom g) {
  const IirBlock blk = slab_block_of(g, blockIdx.x);
  if (!blk.live) return;
  const ZSlabJob &J = jobs.j[blk.job];
  const IirCoef c = J.c;
  SlabLine l;
  if (!slab_line(g, blk.group, l)) return;
  const int64_t n = g.n;
  const int64_t nb = (n + K - 1) / K;
  const int64_t ioff = g.has_lo ? 4 : 0;
  CausalState s;
  float xb[K], xn[K];
  slab_load_block<K>(J.in, g, l.Lw, l.voff, 0, xb);
  if (g.has_lo) {
    y4_load(J.sin_y, g.nlines, l.Lw, l.voff, s.y1, s.y2, s.y3, s.y4);
    float h[3];  // x[-3], x[-2], x[-1]: the last planes of the slab below
    slab_load_planes<3>(J.in, g, l.Lw, l.voff, -3, h);
    s.x1 = (double)h[2]; s.x2 = (double)h[1]; s.x3 = (double)h[0];
  } else {
    const double e0 = (double)xb[0];
    s.x1 = s.x2 = s.x3 = e0;
    s.y1 = s.y2 = s.y3 = s.y4 = e0;
  }
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t i0 = b * K;
    if (b + 1 < nb) slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 + K, xn);
    if (!(b & 1) && l.live)
      y4_store(J.cy + (b / 2) * 4 * g.ck_stride, g.ck_stride, l.Lw, l.voff, s.y1, s.y2, s.y3, s.y4);
    if (i0 + K <= n && (b > 0 || g.has_lo)) {
#pragma unroll
      for (int j = 0; j < K; ++j) causal_step(s, (double)xb[j], c);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (i0 + j < n) causal_step_edge(s, (double)xb[j], c, i0 + j + ioff);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) xb[j] = xn[j];
  }
  if (l.live) y4_store(J.sout_y, g.nlines, l.Lw, l.voff, s.y1, s.y2, s.y3, s.y4);
}

// ---- anticausal sweep: downwards from the state of the slab above (or the end of line) ----
template <int K>
__global__ __launch_bounds__(256) void zslab_anti_kernel(ZSlabJobs jobs, ZSlabGeom g) {
  const IirBlock blk = slab_block_of(g, blockIdx.x);
  if (!blk.live) return;
  const ZSlabJob &J = jobs.j[blk.job];
  const IirCoef c = J.c;
  SlabLine l;
  if (!slab_line(g, blk.group, l)) return;
  const int64_t n = g.n;
  const int64_t nb = (n + K - 1) / K;
  const int64_t nedge = g.has_hi ? n + 8 : n;
  AntiState a;
  float xb[K], xn[K];
  slab_load_block<K>(J.in, g, l.Lw, l.voff, (nb - 1) * K, xb);
  if (g.has_hi) {
    y4_load(J.sin_y, g.nlines, l.Lw, l.voff, a.y1, a.y2, a.y3, a.y4);
    float h[4];  // x[n .. n+3]: the first planes of the slab above
    slab_load_planes<4>(J.in, g, l.Lw, l.voff, n, h);
    a.x1 = (double)h[0]; a.x2 = (double)h[1]; a.x3 = (double)h[2]; a.x4 = (double)h[3];
  } else {
    const double xN = (double)xb[K - 1];  // the clamped load repeats x[n-1]
    a.x1 = a.x2 = a.x3 = a.x4 = xN;
    a.y1 = a.y2 = a.y3 = a.y4 = xN;
  }
  for (int64_t b = nb - 1; b >= 0; --b) {
    const int64_t i0 = b * K;
    if (b > 0) slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 - K, xn);
    if (((b & 1) || b == nb - 1) && l.live)
      y4_store(J.ay + (b / 2) * 4 * g.ck_stride, g.ck_stride, l.Lw, l.voff, a.y1, a.y2, a.y3, a.y4);
    if (i0 + K + 4 <= nedge && i0 + K <= n) {
#pragma unroll
      for (int j = K - 1; j >= 0; --j) anti_step(a, (double)xb[j], c);
    } else {
#pragma unroll
      for (int j = K - 1; j >= 0; --j)
        if (i0 + j < n) anti_step_edge(a, (double)xb[j], c, i0 + j, nedge);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) xb[j] = xn[j];
  }
  if (l.live) y4_store(J.sout_y, g.nlines, l.Lw, l.voff, a.y1, a.y2, a.y3, a.y4);
}

// ---- lean sweeps of three jobs over the same planes (orders 0, 1, 2 of one source) ----------
// The differential path sweeps every source three times with one sigma: the jobs 3t, 3t + 1,
// 3t + 2 of a launch read the same planes.  Here a lane owns one line of one SOURCE (g.njobs
// counts sources): every register block is loaded once and advances the three recursions from
// it -- the x history shared, three y histories, three sets of input coefficients, as
// iir_sweep_z_kernel runs its scales side by side -- and the checkpoints and outgoing states of
// the three jobs go exactly where zslab_causal_kernel / zslab_anti_kernel put them.  Every sample
// sees the operations of the per-job kernels in their order: same bits.  The feedback
// coefficients D1..D4 depend on sigma and spacing only, not on the order: the host sends three
// jobs here only where theirs are the same doubles, and the steady loop keeps one set (32 scalar
// registers of coefficients instead of 48).
// Every memory operation of the pair loop is unconditional.  A block that does not exist is
// replaced by the nearest one that does (its values are not used), rows past the slab's last
// plane repeat that plane, and a lane past the last line computes on the last line; it never
// stores, because every row of a record goes through a descriptor that ends with the launch's
// last line.
struct Sweep4 {
  double k0, k1, k2, k3;  // N0..N3 (causal), M1..M4 (anticausal), D1..D4
};
// the four border coefficients of a slab job (first = 12: BN1..BN4, 16: BM1..BM4), re-read from
// the kernel-argument segment where a border block needs them (edge_coefs, for ZSlabJobs as the
// first argument); the other eight it needs are the steady loop's own
__device__ __forceinline__ Sweep4 slab_border_coefs(uint32_t job, int first) {
  typedef __attribute__((address_space(4))) const char kchar;
  kchar *ka = (kchar *)__builtin_amdgcn_kernarg_segment_ptr() + (size_t)job * sizeof(ZSlabJob) + offsetof(ZSlabJob, c);
  asm volatile("" : "+s"(ka));
  typedef __attribute__((address_space(4))) const double kdouble;
  kdouble *d = (kdouble *)ka + first;
  return Sweep4{d[0], d[1], d[2], d[3]};
}
static_assert(offsetof(IirCoef, BN1) == 12 * sizeof(double) && offsetof(IirCoef, BM1) == 16 * sizeof(double),
              "slab_border_coefs reads IirCoef as 20 doubles");
// causal_step / anti_step with the x history outside the state
__device__ __forceinline__ void sweep3_causal(SweepY &s, double x1, double x2, double x3, double xin,
                                              const Sweep4 &N, const Sweep4 &D) {
  const double a = IFE_MADD(x3, N.k3, IFE_MADD(x2, N.k2, IFE_MADD(x1, N.k1, xin * N.k0)));
  const double t = IFE_MADD(s.y4, D.k3, IFE_MADD(s.y3, D.k2, IFE_MADD(s.y2, D.k1, s.y1 * D.k0)));
  const double y = a - t;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
}
__device__ __forceinline__ void sweep3_anti(SweepY &s, double x1, double x2, double x3, double x4,
                                            const Sweep4 &M, const Sweep4 &D) {
  const double a = IFE_MADD(x4, M.k3, IFE_MADD(x3, M.k2, IFE_MADD(x2, M.k1, x1 * M.k0)));
  const double t = IFE_MADD(s.y4, D.k3, IFE_MADD(s.y3, D.k2, IFE_MADD(s.y2, D.k1, s.y1 * D.k0)));
  const double y = a - t;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
}
// causal_step_edge / anti_step_edge likewise: B are the border coefficients, i (n) as there
__device__ __forceinline__ void sweep3_causal_edge(SweepY &s, double x1, double x2, double x3, double xin,
                                                   const Sweep4 &N, const Sweep4 &D, const Sweep4 &B, int64_t i) {
  const double d1 = i < 1 ? B.k0 : D.k0;
  const double d2 = i < 2 ? B.k1 : D.k1;
  const double d3 = i < 3 ? B.k2 : D.k2;
  const double d4 = i < 4 ? B.k3 : D.k3;
  const double a = IFE_MADD(x3, N.k3, IFE_MADD(x2, N.k2, IFE_MADD(x1, N.k1, xin * N.k0)));
  const double t = IFE_MADD(s.y4, d4, IFE_MADD(s.y3, d3, IFE_MADD(s.y2, d2, s.y1 * d1)));
  const double y = a - t;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
}
__device__ __forceinline__ void sweep3_anti_edge(SweepY &s, double x1, double x2, double x3, double x4,
                                                 const Sweep4 &M, const Sweep4 &D, const Sweep4 &B, int64_t i,
                                                 int64_t n) {
  const double d1 = i + 1 >= n ? B.k0 : D.k0;
  const double d2 = i + 2 >= n ? B.k1 : D.k1;
  const double d3 = i + 3 >= n ? B.k2 : D.k2;
  const double d4 = i + 4 >= n ? B.k3 : D.k3;
  const double a = IFE_MADD(x4, M.k3, IFE_MADD(x3, M.k2, IFE_MADD(x2, M.k1, x1 * M.k0)));
  const double t = IFE_MADD(s.y4, d4, IFE_MADD(s.y3, d3, IFE_MADD(s.y2, d2, s.y1 * d1)));
  const double y = a - t;
  s.y4 = s.y3; s.y3 = s.y2; s.y2 = s.y1; s.y1 = y;
}
// K samples from plane i0 (0 <= i0 < n) of the lane's line, rows past the slab's last plane
// repeating it: slab_load_block without its branch (the row offsets are scalar minima)
template <int K>
__device__ __forceinline__ void slab_load_block_clamped(const float *in, const ZSlabGeom &g, int64_t Lw,
                                                        uint32_t voff, int64_t i0, float (&x)[K]) {
  const rsrc_t r = IFE_IN_RSRC(in + Lw + i0 * g.sstride);
  const uint32_t sst = (uint32_t)g.sstride;
  const int64_t left = g.n - 1 - i0;
  const uint32_t lastj = (uint32_t)(left < K - 1 ? left : K - 1);
#pragma unroll
  for (int j = 0; j < K; ++j)
    x[j] = buf_ld_f32(r, voff * 4u, ((uint32_t)j < lastj ? (uint32_t)j : lastj) * sst * 4u);
}
// One record [4][stride] of a live lane; `live_bytes` = 8 * (lines of this wave inside the
// launch): the lanes past them fall outside every row's descriptor and their stores are dropped
__device__ __forceinline__ void y4_store_live(double *y, int64_t stride, int64_t Lw, uint32_t lane,
                                              uint32_t live_bytes, const SweepY &s) {
  double *const base = reinterpret_cast<double *>(uniform64(reinterpret_cast<int64_t>(y))) + Lw;
  buf_st_f64(make_rsrc_range(base, live_bytes), lane * 8u, 0u, s.y1);
  buf_st_f64(make_rsrc_range(base + stride, live_bytes), lane * 8u, 0u, s.y2);
  buf_st_f64(make_rsrc_range(base + 2 * stride, live_bytes), lane * 8u, 0u, s.y3);
  buf_st_f64(make_rsrc_range(base + 3 * stride, live_bytes), lane * 8u, 0u, s.y4);
}

// (three waves per SIMD: held to four, the three chains spill to scratch inside the steady block
// and the sweep of a 512 x 512 x 64 slab takes 0.093 ms instead of 0.082)
template <int K>
__global__ __launch_bounds__(256) void zslab_causal3_kernel(ZSlabJobs jobs, ZSlabGeom g) {
  const IirBlock blk = slab_block_of(g, blockIdx.x);  // g.njobs = sources: blk.job is the source
  if (!blk.live) return;
  SlabLine l;
  if (!slab_line(g, blk.group, l)) return;
  const uint32_t j0 = blk.job * 3u;
  const int64_t n = g.n;
  const int64_t nb = (n + K - 1) / K;
  const int64_t np = (nb + 1) / 2;
  const int64_t ioff = g.has_lo ? 4 : 0;
  const int64_t rest = g.nlines - l.Lw;  // >= 1 (slab_line)
  const uint32_t live_bytes = (uint32_t)(rest < 64 ? rest : 64) * 8u;
  const float *const in = jobs.j[j0].in;  // the three jobs read the same planes (the host's test)
  Sweep4 N[3];
  double *cy[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const ZSlabJob &J = jobs.j[j0 + k];
    N[k] = Sweep4{J.c.N0, J.c.N1, J.c.N2, J.c.N3};
    cy[k] = J.cy;
  }
  const Sweep4 D = {jobs.j[j0].c.D1, jobs.j[j0].c.D2, jobs.j[j0].c.D3, jobs.j[j0].c.D4};
  SweepY s[3];
  double x1, x2, x3;
  float xb[K], xn[K];
  slab_load_block_clamped<K>(in, g, l.Lw, l.voff, 0, xb);
  if (g.has_lo) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      y4_load(jobs.j[j0 + k].sin_y, g.nlines, l.Lw, l.voff, s[k].y1, s[k].y2, s[k].y3, s[k].y4);
    float h[3];  // x[-3], x[-2], x[-1]: the last planes of the slab below
    slab_load_planes<3>(in, g, l.Lw, l.voff, -3, h);
    x1 = (double)h[2]; x2 = (double)h[1]; x3 = (double)h[0];
  } else {
    const double e0 = (double)xb[0];
    x1 = x2 = x3 = e0;
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = SweepY{e0, e0, e0, e0};
  }
  // the recursions over the block in xb, which starts at plane i0 (uniform branches over
  // arithmetic only).  The border form where zslab_causal_kernel takes it, one job after the
  // other, each with its border coefficients and its own copy of the x history.
  auto run = [&](int64_t i0, bool first) {
    if (i0 + K <= n && !first) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        // (scheduling fence: left alone, the conversions of the whole block move to its front)
        if (j % IFE_IIR_FENCE == 0) __builtin_amdgcn_sched_barrier(0);
        const double xin = (double)xb[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) sweep3_causal(s[k], x1, x2, x3, xin, N[k], D);
        x3 = x2; x2 = x1; x1 = xin;
      }
    } else {
      double e1 = x1, e2 = x2, e3 = x3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const Sweep4 B = slab_border_coefs(j0 + (uint32_t)k, 12);
        e1 = x1; e2 = x2; e3 = x3;
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (i0 + j < n) {
            const double xin = (double)xb[j];
            sweep3_causal_edge(s[k], e1, e2, e3, xin, N[k], D, B, i0 + j + ioff);
            e3 = e2; e2 = e1; e1 = xin;
          }
      }
      x1 = e1; x2 = e2; x3 = e3;
    }
  };
  for (int64_t p = 0; p < np; ++p) {
    const int64_t iA = 2 * p * K, iB = iA + K;
    const bool hasB = iB < n;
    const int64_t iBe = hasB ? iB : iA;  // the pair's last block that exists
    slab_load_block_clamped<K>(in, g, l.Lw, l.voff, iBe, xn);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      y4_store_live(cy[k] + p * 4 * g.ck_stride, g.ck_stride, l.Lw, l.lane, live_bytes, s[k]);
    run(iA, p == 0 && !g.has_lo);
#pragma unroll
    for (int j = 0; j < K; ++j) xb[j] = xn[j];
    slab_load_block_clamped<K>(in, g, l.Lw, l.voff, iB + K < n ? iB + K : iBe, xn);
    if (hasB) run(iB, false);
#pragma unroll
    for (int j = 0; j < K; ++j) xb[j] = xn[j];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) y4_store_live(jobs.j[j0 + k].sout_y, g.nlines, l.Lw, l.lane, live_bytes, s[k]);
}

// (four waves per SIMD, without scratch in the exact build: two sources of a 512 x 512 slab are
// eight waves per SIMD, two full rounds)
template <int K>
__global__ __launch_bounds__(256, 4) void zslab_anti3_kernel(ZSlabJobs jobs, ZSlabGeom g) {
  const IirBlock blk = slab_block_of(g, blockIdx.x);  // g.njobs = sources: blk.job is the source
  if (!blk.live) return;
  SlabLine l;
  if (!slab_line(g, blk.group, l)) return;
  const uint32_t j0 = blk.job * 3u;
  const int64_t n = g.n;
  const int64_t nb = (n + K - 1) / K;
  const int64_t np = (nb + 1) / 2;
  const int64_t nedge = g.has_hi ? n + 8 : n;
  const int64_t rest = g.nlines - l.Lw;  // >= 1 (slab_line)
  const uint32_t live_bytes = (uint32_t)(rest < 64 ? rest : 64) * 8u;
  const float *const in = jobs.j[j0].in;
  Sweep4 M[3];
  double *ay[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const ZSlabJob &J = jobs.j[j0 + k];
    M[k] = Sweep4{J.c.M1, J.c.M2, J.c.M3, J.c.M4};
    ay[k] = J.ay;
  }
  const Sweep4 D = {jobs.j[j0].c.D1, jobs.j[j0].c.D2, jobs.j[j0].c.D3, jobs.j[j0].c.D4};
  SweepY a[3];
  double x1, x2, x3, x4;
  float xb[K], xn[K];
  slab_load_block_clamped<K>(in, g, l.Lw, l.voff, (nb - 1) * K, xb);
  if (g.has_hi) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      y4_load(jobs.j[j0 + k].sin_y, g.nlines, l.Lw, l.voff, a[k].y1, a[k].y2, a[k].y3, a[k].y4);
    float h[4];  // x[n .. n+3]: the first planes of the slab above
    slab_load_planes<4>(in, g, l.Lw, l.voff, n, h);
    x1 = (double)h[0]; x2 = (double)h[1]; x3 = (double)h[2]; x4 = (double)h[3];
  } else {
    const double xN = (double)xb[K - 1];  // the clamped load repeats x[n-1]
    x1 = x2 = x3 = x4 = xN;
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = SweepY{xN, xN, xN, xN};
  }
  auto run = [&](int64_t i0) {
    if (i0 + K + 4 <= nedge && i0 + K <= n) {
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        if (j % IFE_IIR_FENCE == 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 3; ++k) sweep3_anti(a[k], x1, x2, x3, x4, M[k], D);
        x4 = x3; x3 = x2; x2 = x1; x1 = (double)xb[j];
      }
    } else {
      double e1 = x1, e2 = x2, e3 = x3, e4 = x4;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const Sweep4 B = slab_border_coefs(j0 + (uint32_t)k, 16);
        e1 = x1; e2 = x2; e3 = x3; e4 = x4;
#pragma unroll
        for (int j = K - 1; j >= 0; --j)
          if (i0 + j < n) {
            sweep3_anti_edge(a[k], e1, e2, e3, e4, M[k], D, B, i0 + j, nedge);
            e4 = e3; e3 = e2; e2 = e1; e1 = (double)xb[j];
          }
      }
      x1 = e1; x2 = e2; x3 = e3; x4 = e4;
    }
  };
  for (int64_t p = np - 1; p >= 0; --p) {
    const int64_t iA = 2 * p * K, iB = iA + K;
    const bool hasB = iB < n;  // false for the line's last pair at most
    // xb holds the pair's last block that exists; its checkpoint lies in front of that block
    slab_load_block_clamped<K>(in, g, l.Lw, l.voff, iA, xn);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      y4_store_live(ay[k] + p * 4 * g.ck_stride, g.ck_stride, l.Lw, l.lane, live_bytes, a[k]);
    if (hasB) {
      run(iB);
#pragma unroll
      for (int j = 0; j < K; ++j) xb[j] = xn[j];
    }
    slab_load_block_clamped<K>(in, g, l.Lw, l.voff, p > 0 ? iA - K : iA, xn);
    run(iA);
#pragma unroll
    for (int j = 0; j < K; ++j) xb[j] = xn[j];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) y4_store_live(jobs.j[j0 + k].sout_y, g.nlines, l.Lw, l.lane, live_bytes, a[k]);
}

// ---- combine: both recursions of every pair from its two checkpoints, summed and stored ----
template <int K>
__global__ __launch_bounds__(256, 3) void zslab_combine_kernel(ZSlabJobs jobs, ZSlabGeom g) {
  const IirBlock blk = slab_block_of(g, blockIdx.x);
  if (!blk.live) return;
  const ZSlabJob &J = jobs.j[blk.job];
  const IirCoef c = J.c;
  SlabLine l;
  if (!slab_line(g, blk.group, l)) return;
  __shared__ double park[4][2 * K][64];
  double *col = &park[threadIdx.x >> 6][0][l.lane];
  const int64_t n = g.n;
  const int64_t nb = (n + K - 1) / K;
  const int64_t np = (nb + 1) / 2;
  const int64_t ioff = g.has_lo ? 4 : 0;
  const int64_t nedge = g.has_hi ? n + 8 : n;
  const uint32_t sst = (uint32_t)g.sstride;
  float xa[K], xb[K], na[K], nb2[K];
  CausalState s;
  AntiState a;
  double ncy[4], nay[4];       // y checkpoints of the next pair, in flight
  float xlo[3] = {0.f, 0.f, 0.f}, xhi[4] = {0.f, 0.f, 0.f, 0.f};
  slab_load_block<K>(J.in, g, l.Lw, l.voff, 0, xa);
  slab_load_block<K>(J.in, g, l.Lw, l.voff, K < n ? K : 0, xb);
  y4_load(J.cy, g.ck_stride, l.Lw, l.voff, s.y1, s.y2, s.y3, s.y4);
  y4_load(J.ay, g.ck_stride, l.Lw, l.voff, a.y1, a.y2, a.y3, a.y4);
  if (g.has_lo) slab_load_planes<3>(J.in, g, l.Lw, l.voff, -3, xlo);  // x[-3], x[-2], x[-1]
  if (g.has_hi) slab_load_planes<4>(J.in, g, l.Lw, l.voff, n, xhi);   // x[n .. n+3]
  if (g.has_lo) {
    s.x1 = (double)xlo[2]; s.x2 = (double)xlo[1]; s.x3 = (double)xlo[0];
  } else {
    s.x1 = s.x2 = s.x3 = (double)xa[0];  // ITK's start of line
  }
  // x[k] for k >= n: the slab above (its first samples) or, at the end of the line, x[n-1]
  auto beyond = [&](int64_t k, float clamped) {
    const int64_t d = k - n;  // 0..3; selects instead of a dynamically indexed register array
    const float v = d == 0 ? xhi[0] : d == 1 ? xhi[1] : d == 2 ? xhi[2] : xhi[3];
    return g.has_hi ? v : clamped;
  };
  for (int64_t p = 0; p < np; ++p) {
    const int64_t i0 = 2 * p * K, i1 = i0 + K;
    const bool more = p + 1 < np;
    if (more) {  // the next pair's samples and checkpoints, in flight across this pair
      slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 + 2 * K, na);
      slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 + 3 * K < n ? i0 + 3 * K : i0 + 2 * K, nb2);
      y4_load(J.cy + (p + 1) * 4 * g.ck_stride, g.ck_stride, l.Lw, l.voff, ncy[0], ncy[1], ncy[2], ncy[3]);
      y4_load(J.ay + (p + 1) * 4 * g.ck_stride, g.ck_stride, l.Lw, l.voff, nay[0], nay[1], nay[2], nay[3]);
    }
    // x history of the anticausal state in front of this pair's last sample: the four
    // samples above it, which are the next pair's first ones where the slab has them
    {
      const int64_t top = (i0 + 2 * K < n ? i0 + 2 * K : n) - 1;
      float xt[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t idx = top + 1 + k;
        // inside the slab idx >= i0 + 2K, so it is sample idx - (i0 + 2K) of the next pair's
        // first block (K >= 4); the clamped load already repeats x[n-1] past the end
        const float in_slab = more ? na[k] : xb[K - 1];
        xt[k] = idx < n ? in_slab : beyond(idx, more ? na[k] : (i1 < n ? xb[K - 1] : xa[K - 1]));
      }
      a.x1 = (double)xt[0]; a.x2 = (double)xt[1]; a.x3 = (double)xt[2]; a.x4 = (double)xt[3];
    }
    // x history of the NEXT pair's causal state: this pair's last three samples (the pair is
    // complete whenever a next one exists); taken before the outputs overwrite the registers
    const float nh1 = xb[K - 1], nh2 = xb[K - 2], nh3 = xb[K - 3];
    const bool inner = i0 + 2 * K + 4 <= nedge && i0 + 2 * K <= n && (p > 0 || g.has_lo);
    const rsrc_t ro = IFE_OUT_RSRC(J.out + l.Lw + i0 * g.sstride);
    if (inner) {
#pragma unroll
      for (int j = 0; j < K; ++j) col[j * 64] = causal_step(s, (double)xa[j], c);
#pragma unroll
      for (int j = 0; j < K; ++j) col[(K + j) * 64] = causal_step(s, (double)xb[j], c);
#pragma unroll
      for (int j = K - 1; j >= 0; --j) xb[j] = (float)(col[(K + j) * 64] + anti_step(a, (double)xb[j], c));
#pragma unroll
      for (int j = K - 1; j >= 0; --j) xa[j] = (float)(col[j * 64] + anti_step(a, (double)xa[j], c));
      if (l.live) {
#pragma unroll
        for (int j = 0; j < K; ++j) buf_st_out_f32(ro, l.voff * 4u, (uint32_t)j * sst * 4u, xa[j]);
#pragma unroll
        for (int j = 0; j < K; ++j) buf_st_out_f32(ro, l.voff * 4u, (uint32_t)(K + j) * sst * 4u, xb[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (i0 + j < n) col[j * 64] = causal_step_edge(s, (double)xa[j], c, i0 + j + ioff);
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (i1 + j < n) col[(K + j) * 64] = causal_step_edge(s, (double)xb[j], c, i1 + j + ioff);
#pragma unroll
      for (int j = K - 1; j >= 0; --j)
        if (i1 + j < n) xb[j] = (float)(col[(K + j) * 64] + anti_step_edge(a, (double)xb[j], c, i1 + j, nedge));
#pragma unroll
      for (int j = K - 1; j >= 0; --j)
        if (i0 + j < n) xa[j] = (float)(col[j * 64] + anti_step_edge(a, (double)xa[j], c, i0 + j, nedge));
      if (l.live) {
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (i0 + j < n) buf_st_out_f32(ro, l.voff * 4u, (uint32_t)j * sst * 4u, xa[j]);
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (i1 + j < n) buf_st_out_f32(ro, l.voff * 4u, (uint32_t)(K + j) * sst * 4u, xb[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) { xa[j] = na[j]; xb[j] = nb2[j]; }
    s.y1 = ncy[0]; s.y2 = ncy[1]; s.y3 = ncy[2]; s.y4 = ncy[3];
    s.x1 = (double)nh1; s.x2 = (double)nh2; s.x3 = (double)nh3;
    a.y1 = nay[0]; a.y2 = nay[1]; a.y3 = nay[2]; a.y4 = nay[3];
  }
}

// ---- fused: one recursion carried through the slab, the other rebuilt from checkpoints ----
// The direction whose state reaches a rank LAST does not need a lean sweep of its own: once
// that state is there, the recursion can run through the slab from it and take the other
// direction's values, pair by pair, from the checkpoints the lean sweep of that other direction
// left (DIR 0: causal carried upwards, anticausal from `ay`; DIR 1: anticausal carried
// downwards, causal from `cy`).  It writes the pass's output and hands the carried state on.
// Per sample that is 1 (lean sweep of the early direction) + 2 (this kernel) recursion steps
// instead of 1 + 1 + 2 with two sweeps and a combine; every sample still sees exactly the
// operations of the sequential recursion.
template <int K, int DIR>
__global__ __launch_bounds__(256, 3) void zslab_fused_kernel(ZSlabJobs jobs, ZSlabGeom g) {
  const IirBlock blk = slab_block_of(g, blockIdx.x);
  if (!blk.live) return;
  const ZSlabJob &J = jobs.j[blk.job];
  const IirCoef c = J.c;
  SlabLine l;
  if (!slab_line(g, blk.group, l)) return;
  __shared__ double park[4][2 * K][64];
  double *col = &park[threadIdx.x >> 6][0][l.lane];
  const int64_t n = g.n;
  const int64_t nb = (n + K - 1) / K;
  const int64_t np = (nb + 1) / 2;
  const int64_t ioff = g.has_lo ? 4 : 0;
  const int64_t nedge = g.has_hi ? n + 8 : n;
  const uint32_t sst = (uint32_t)g.sstride;
  float xa[K], xb[K], na[K], nb2[K];
  CausalState s;
  AntiState a;
  double nck[4];  // checkpoint of the next pair (the direction that is NOT carried), in flight
  float xlo[3] = {0.f, 0.f, 0.f}, xhi[4] = {0.f, 0.f, 0.f, 0.f};
  if (g.has_lo) slab_load_planes<3>(J.in, g, l.Lw, l.voff, -3, xlo);  // x[-3], x[-2], x[-1]
  if (g.has_hi) slab_load_planes<4>(J.in, g, l.Lw, l.voff, n, xhi);   // x[n .. n+3]
  // x[k] for k >= n: the slab above (its first samples) or, at the end of the line, x[n-1]
  auto beyond = [&](int64_t k, float clamped) {
    const int64_t d = k - n;  // 0..3; selects instead of a dynamically indexed register array
    const float v = d == 0 ? xhi[0] : d == 1 ? xhi[1] : d == 2 ? xhi[2] : xhi[3];
    return g.has_hi ? v : clamped;
  };
  // both recursions over one pair held in xa / xb, outputs stored; `s` and `a` enter with the
  // states in front of the pair's first / behind its last sample and leave with those behind it.
  // Border coefficients and ragged ends are decided per BLOCK and recursion, not per pair: of
  // the 2 2/3 pairs of a 64-plane slab only the 4 samples of the last block (and, on the first
  // or last rank, the block at the line's end) take the index-tested form.
  auto pair_body = [&](int64_t p) {
    const int64_t i0 = 2 * p * K, i1 = i0 + K;
    const bool fullA = i0 + K <= n, fullB = i1 + K <= n, hasB = i1 < n;
    const bool cA_plain = fullA && (p > 0 || g.has_lo);  // no sample with index (+ioff) < 4
    const bool cB_plain = fullB;                          // i1 >= K >= 4
    const bool aB_plain = fullB && i1 + K + 4 <= nedge;   // no sample within 4 of the line's end
    const bool aA_plain = fullA && i0 + K + 4 <= nedge;
    const rsrc_t ro = IFE_OUT_RSRC(J.out + l.Lw + i0 * g.sstride);
    if (cA_plain) {
#pragma unroll
      for (int j = 0; j < K; ++j) col[j * 64] = causal_step(s, (double)xa[j], c);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (i0 + j < n) col[j * 64] = causal_step_edge(s, (double)xa[j], c, i0 + j + ioff);
    }
    if (cB_plain) {
#pragma unroll
      for (int j = 0; j < K; ++j) col[(K + j) * 64] = causal_step(s, (double)xb[j], c);
    } else if (hasB) {
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (i1 + j < n) col[(K + j) * 64] = causal_step_edge(s, (double)xb[j], c, i1 + j + ioff);
    }
    if (aB_plain) {
#pragma unroll
      for (int j = K - 1; j >= 0; --j) xb[j] = (float)(col[(K + j) * 64] + anti_step(a, (double)xb[j], c));
    } else if (hasB) {
#pragma unroll
      for (int j = K - 1; j >= 0; --j)
        if (i1 + j < n) xb[j] = (float)(col[(K + j) * 64] + anti_step_edge(a, (double)xb[j], c, i1 + j, nedge));
    }
    if (aA_plain) {
#pragma unroll
      for (int j = K - 1; j >= 0; --j) xa[j] = (float)(col[j * 64] + anti_step(a, (double)xa[j], c));
    } else {
#pragma unroll
      for (int j = K - 1; j >= 0; --j)
        if (i0 + j < n) xa[j] = (float)(col[j * 64] + anti_step_edge(a, (double)xa[j], c, i0 + j, nedge));
    }
    if (fullA) {
#pragma unroll
      for (int j = 0; j < K; ++j) buf_st_out_f32(ro, l.voff * 4u, (uint32_t)j * sst * 4u, xa[j]);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (i0 + j < n) buf_st_out_f32(ro, l.voff * 4u, (uint32_t)j * sst * 4u, xa[j]);
    }
    if (fullB) {
#pragma unroll
      for (int j = 0; j < K; ++j) buf_st_out_f32(ro, l.voff * 4u, (uint32_t)(K + j) * sst * 4u, xb[j]);
    } else if (hasB) {
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (i1 + j < n) buf_st_out_f32(ro, l.voff * 4u, (uint32_t)(K + j) * sst * 4u, xb[j]);
    }
  };

  if constexpr (DIR == 0) {
    // ---- causal carried upwards from the state of the slab below; anticausal from `ay` ----
    slab_load_block<K>(J.in, g, l.Lw, l.voff, 0, xa);
    slab_load_block<K>(J.in, g, l.Lw, l.voff, K < n ? K : 0, xb);
    y4_load(J.ay, g.ck_stride, l.Lw, l.voff, a.y1, a.y2, a.y3, a.y4);
    if (g.has_lo) {
      y4_load(J.sin_y, g.nlines, l.Lw, l.voff, s.y1, s.y2, s.y3, s.y4);
      s.x1 = (double)xlo[2]; s.x2 = (double)xlo[1]; s.x3 = (double)xlo[0];
    } else {
      const double e0 = (double)xa[0];  // ITK's start of line
      s.x1 = s.x2 = s.x3 = e0;
      s.y1 = s.y2 = s.y3 = s.y4 = e0;
    }
    for (int64_t p = 0; p < np; ++p) {
      const int64_t i0 = 2 * p * K, i1 = i0 + K;
      const bool more = p + 1 < np;
      if (more) {  // the next pair's samples and anticausal checkpoint, in flight across this pair
        slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 + 2 * K, na);
        slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 + 3 * K < n ? i0 + 3 * K : i0 + 2 * K, nb2);
        y4_load(J.ay + (p + 1) * 4 * g.ck_stride, g.ck_stride, l.Lw, l.voff, nck[0], nck[1], nck[2], nck[3]);
      }
      // x history of the anticausal state in front of this pair's last sample: the four
      // samples above it (zslab_combine_kernel)
      {
        const int64_t top = (i0 + 2 * K < n ? i0 + 2 * K : n) - 1;
        float xt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t idx = top + 1 + k;
          const float in_slab = more ? na[k] : xb[K - 1];
          xt[k] = idx < n ? in_slab : beyond(idx, more ? na[k] : (i1 < n ? xb[K - 1] : xa[K - 1]));
        }
        a.x1 = (double)xt[0]; a.x2 = (double)xt[1]; a.x3 = (double)xt[2]; a.x4 = (double)xt[3];
      }
      pair_body(p);
#pragma unroll
      for (int j = 0; j < K; ++j) { xa[j] = na[j]; xb[j] = nb2[j]; }
      a.y1 = nck[0]; a.y2 = nck[1]; a.y3 = nck[2]; a.y4 = nck[3];
    }
    if (l.live) y4_store(J.sout_y, g.nlines, l.Lw, l.voff, s.y1, s.y2, s.y3, s.y4);
  } else {
    // ---- anticausal carried downwards from the state of the slab above; causal from `cy` ----
    {
      const int64_t i0 = 2 * (np - 1) * K;
      slab_load_block<K>(J.in, g, l.Lw, l.voff, i0, xa);
      slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 + K < n ? i0 + K : i0, xb);
      y4_load(J.cy + (np - 1) * 4 * g.ck_stride, g.ck_stride, l.Lw, l.voff, s.y1, s.y2, s.y3, s.y4);
      if (g.has_hi) {
        y4_load(J.sin_y, g.nlines, l.Lw, l.voff, a.y1, a.y2, a.y3, a.y4);
        a.x1 = (double)xhi[0]; a.x2 = (double)xhi[1]; a.x3 = (double)xhi[2]; a.x4 = (double)xhi[3];
      } else {
        // x[n-1]: the clamped loads repeat it in every slot past the end of the line
        const double xN = (double)(i0 + K < n ? xb[K - 1] : xa[K - 1]);
        a.x1 = a.x2 = a.x3 = a.x4 = xN;
        a.y1 = a.y2 = a.y3 = a.y4 = xN;
      }
    }
    // x history of the causal state in front of a pair: the three samples below it (the slab
    // below's last planes for pair 0), requested a pair ahead like the samples themselves
    float h[3] = {0.f, 0.f, 0.f}, nh[3] = {0.f, 0.f, 0.f};
    if (np > 1 || g.has_lo) slab_load_planes<3>(J.in, g, l.Lw, l.voff, 2 * (np - 1) * K - 3, h);
    for (int64_t p = np - 1; p >= 0; --p) {
      const int64_t i0 = 2 * p * K;
      if (p > 0) {  // the pair below (always complete), its causal checkpoint and history, in flight
        slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 - 2 * K, na);
        slab_load_block<K>(J.in, g, l.Lw, l.voff, i0 - K, nb2);
        y4_load(J.cy + (p - 1) * 4 * g.ck_stride, g.ck_stride, l.Lw, l.voff, nck[0], nck[1], nck[2], nck[3]);
        if (p > 1 || g.has_lo) slab_load_planes<3>(J.in, g, l.Lw, l.voff, i0 - 2 * K - 3, nh);
      }
      if (p > 0 || g.has_lo) {
        s.x1 = (double)h[2]; s.x2 = (double)h[1]; s.x3 = (double)h[0];
      } else {
        s.x1 = s.x2 = s.x3 = (double)xa[0];  // ITK's start of line
      }
      pair_body(p);
#pragma unroll
      for (int j = 0; j < K; ++j) { xa[j] = na[j]; xb[j] = nb2[j]; }
      h[0] = nh[0]; h[1] = nh[1]; h[2] = nh[2];
      s.y1 = nck[0]; s.y2 = nck[1]; s.y3 = nck[2]; s.y4 = nck[3];
    }
    if (l.live) y4_store(J.sout_y, g.nlines, l.Lw, l.voff, a.y1, a.y2, a.y3, a.y4);
  }
}


}  // namespace IFE_IIR_NS
}  // namespace ife
#undef IFE_MADD
