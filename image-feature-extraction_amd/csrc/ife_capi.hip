// ife_capi.hip -- C-ABI (include/ife_hip.h) over the HIP kernels.  gfx950 only.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// (-ffp-contract=off is part of the numerical contract, see iir_kernels.inc).
#include "../../include/ife_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "feature_kernels.hpp"
#include "iir_types.hpp"
#include "stats_kernels.hpp"
#include "distance_kernels.hpp"
#include "dense_kernels.hpp"
#include "dense_plan.hpp"
#include "labels_kernels.hpp"
#include "deflate_kernels.hpp"
#include "resample_kernels.hpp"
#include "bspline_kernels.hpp"
#include "region_kernels.hpp"
#include "sampling_kernels.hpp"
#include "coverage_kernels.hpp"
#include "scale_select_kernels.hpp"
#define IFE_IIR_NS iir_exact
#define IFE_IIR_FMA 0
#include "iir_kernels.inc"
#undef IFE_IIR_NS
#undef IFE_IIR_FMA
#define IFE_IIR_NS iir_fma
#define IFE_IIR_FMA 1
#include "iir_kernels.inc"
#undef IFE_IIR_NS
#undef IFE_IIR_FMA

using namespace ife;

namespace {

// The line kernels of one build of iir_kernels.inc (exact or fused multiply-add), as a type:
// the launchers take it as a template parameter.
#define IFE_IIR_KERNELS(NS)                                                                      \
  struct NS##_kernels {                                                                          \
    template <int K> static constexpr auto contig = NS::iir_contig_kernel<K>;                    \
    template <int K> static constexpr auto strided1 = NS::iir_strided1_kernel<K>;                \
    template <int K, bool PAIRED, bool BWD> static constexpr auto strided = NS::iir_strided_kernel<K, PAIRED, BWD>; \
    template <int K, int S, typename TI, typename TM> static constexpr auto sweep_z = NS::iir_sweep_z_kernel<K, S, TI, TM>; \
    template <int K> static constexpr auto zslab_causal = NS::zslab_causal_kernel<K>;            \
    template <int K> static constexpr auto zslab_anti = NS::zslab_anti_kernel<K>;                \
    template <int K> static constexpr auto zslab_causal3 = NS::zslab_causal3_kernel<K>;          \
    template <int K> static constexpr auto zslab_anti3 = NS::zslab_anti3_kernel<K>;              \
    template <int K, int DIR> static constexpr auto zslab_fused = NS::zslab_fused_kernel<K, DIR>; \
    template <int K> static constexpr auto zslab_combine = NS::zslab_combine_kernel<K>;          \
  }
IFE_IIR_KERNELS(iir_exact);
IFE_IIR_KERNELS(iir_fma);
#undef IFE_IIR_KERNELS
template <typename F>
void with_iir_kernels(int fma, F &&f) {
  if (fma) f(iir_fma_kernels{});
  else f(iir_exact_kernels{});
}

// Run-time value to template argument: f(std::integral_constant<int, V>) for the V of the list
// that equals v, for the last of the list when none does.
template <int V0, int... Vs, typename F>
void with_const(int v, F &&f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
  else if (v == V0) f(std::integral_constant<int, V0>{});
  else with_const<Vs...>(v, f);
}

enum KernelKind {
  KK_IIR_Z = 0,
  KK_IIR_X,
  KK_IIR_Y,
  KK_ZSLAB_SWEEP,
  KK_ZSLAB_COMBINE,
  KK_FEATURES,
  KK_EIG_BATCH,
  KK_DIVIDE,
  KK_MASK,
  KK_PREP,
  KK_SORT_HIST,
  KK_SORT_SCAN,
  KK_SORT_SCATTER,
  KK_GATHER,
  KK_EDGES,
  KK_HIST,
  KK_EDT_X,
  KK_EDT_Y,
  KK_EDT_Z,
  KK_EDT_REDUCE,
  KK_DENSE_CODE,
  KK_DENSE_XY,
  KK_DENSE_Z,
  KK_JET,
  KK_COUNT
};
static_assert(KK_COUNT <= IFE_MAX_KERNEL_KINDS, "ife_get_kernel_times callers size their arrays by IFE_MAX_KERNEL_KINDS");
const char *kKindNames[KK_COUNT] = {"iir_z", "iir_x", "iir_y", "zslab_sweep", "zslab_combine", "features", "eig_batch",
                                    "divide", "mask_f64", "prep", "sort_hist", "sort_scan",
                                    "sort_scatter", "gather", "edges", "dense_histogram", "edt_x", "edt_y",
                                    "edt_z", "edt_reduce", "dense_code", "dense_box_xy", "dense_box_z", "jet_features"};

// A device allocation and its owner: move-only, freed by reset() or the destructor (hipFree finds
// the allocation's device, whichever is current).
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  // by exchange: the old allocation is freed with o
  DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~DevBuf() { (void)reset(); }
  hipError_t reset() {
    cap = 0;
    return p ? hipFree(std::exchange(p, nullptr)) : hipSuccess;
  }
  // A fresh allocation in place of the old one, whose contents go; nothing in flight may still
  // use the old one (the caller sees to that).
  hipError_t grow(size_t bytes) {
    hipError_t e = reset();
    if (e == hipSuccess && (e = hipMalloc(&p, bytes)) == hipSuccess) cap = bytes;
    else p = nullptr;
    return e;
  }
};
constexpr int IFE_MAX_SLOTS = 3;

struct ProfRec {
  int kind;
  hipEvent_t a, b;
};

thread_local std::string g_create_error;

}  // namespace

struct ife_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int trig_mode = 2;  // IFE_OPT_TRIG_MODE: float trigonometry inside the 1e-5 bar (ife_hip.h)
  int dscale_mode = 0;
  int profile = 0;
  int zchunk = 64;
  int iir_block = 0;   // 0: per axis (z 12, y 12, x 16); else 8 | 10 | 12 | 16
  int iir_fma = 0;   // 1: fused multiply-add in the line recurrences (opt-in, not bit-exact)
  int iir_ckpt = 2;  // register blocks per checkpoint of the strided line kernel: 1 or 2
  int fused_divide = 1;  // last axis pass stores numerator / denominator (sibling waves), not two fields
  int const_lines = 1;   // lines of one repeated 0 or 1 are copied, not filtered, where verified exact
  int feat_ring = 1;     // feature kernel: planes by LDS-DMA into a ring where the source is one float field
  int z_sweep = 1;       // first axis pass: one causal sweep for all scales from image and mask, no prepass
  int differential = 0;  // IFE_OPT_DIFFERENTIAL: the composite calls take their features from the jet
  std::map<std::tuple<double, double, int64_t>, uint32_t> const_flags;  // (sigma, spacing, length) -> IirJob::const_lines
  // per scale slot: numerator ping/pong, denominator ping/pong (up to three scales run
  // through the line kernels together)
  DevBuf fld[IFE_MAX_SLOTS][4];
  DevBuf pre[2];  // image*certainty and certainty as float (prepass, shared by all scales)
  DevBuf ck_y[IIR_MAX_JOBS];  // one checkpoint area per concurrent job
  DevBuf zs_rec;  // shared Z sweep: constant-line record per field and line (IirJob::line_rec)
  DevBuf st_img, st_mask, st_aux, st_out;  // HOST-mode staging
  // distance map: candidate stacks of the line passes (values, indices), the squared map and
  // the per-line partial sums of the expected distance
  DevBuf edt_g, edt_i, edt_d2, edt_part;
  // dense bag: centre flags and numbers, the scratch of the box passes, clamped labels and features
  DevBuf dn_centres, dn_ws, dn_feat;
  int dense_scratch_mb = 0;  // IFE_OPT_DENSE_SCRATCH_MB: 0 = sized from the free device memory
  // dense bag as a stream of row blocks (ife_bag_dense_stream_*, dense_capi.inc): everything the
  // stream needs between calls is its own, so other calls on the context do not disturb it
  struct DenseStream {
    bool open = false;
    DevBuf codes;    // [ncol][nvox] bin codes of every (scale, feature)
    DevBuf centres;  // centre flags and segment bases (dense_centres)
    DevBuf ws;       // scratch of the box passes of one block
    DevBuf planar;   // the block the z pass fills: [ncol * nb][ld]
    DevBuf rows[2];  // row-major blocks on their way to the host, block k in rows[k % 2]
    hipEvent_t done[2] = {nullptr, nullptr};  // rows[i] is complete
    hipStream_t copy = nullptr;               // device-to-host copies beside the counting of the next block
    std::vector<DenseBlock> blocks;
    size_t next = 0, counted = 0;  // next block to deliver; blocks whose counting is enqueued
    DenseGeom g;
    const uint8_t *flag = nullptr;
    const uint32_t *seg_base = nullptr;
    int ncol = 0, nb = 0, values = 0, cg = 0, bg = 0;
    int64_t n_rois = 0, ld = 0;
  } ds;
  DevBuf dj_ws;  // differential convolution: the field slots of one scale (diff_capi.inc)
  DevBuf ss_ws;  // scale selection: one planar scale of features (scale_select_capi.inc)
  // streaming form of the scale loop (ife_emphysema_features_begin / _fetch / _end)
  DevBuf sc_out;                     // all scales, device resident
  std::vector<hipEvent_t> sc_done;   // one per scale: its feature launch has finished
  hipStream_t sc_copy = nullptr;     // device-to-host copies beside the kernels of later scales
  size_t sc_scale_bytes = 0;
  int sc_layout = IFE_INTERLEAVED;   // of the stream's _begin: the deflated fetch needs whole planes
  // DEFLATE on the device (deflate_capi.inc): offsets, counts and CRC pieces of the chunks, and the
  // blocks of a plane of the stream on their way to the host
  DevBuf df_ws, df_out;
  // resampling (resample_capi.inc): the three axis tables on the device, their host copy (which
  // an upload in flight still reads) and the event behind that upload
  DevBuf rs_tab;
  std::vector<ResampleEntry> rs_host;
  hipEvent_t rs_up = nullptr;
  // B-spline resampling (bspline_capi.inc): the coefficients of the source (8 bytes per voxel), the
  // gather's tables on the device, their host copy and the event behind its upload
  DevBuf bs_coef, bs_tab;
  std::vector<double> bs_host;
  hipEvent_t bs_up = nullptr;
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> ev_pool;
  double acc_ms[KK_COUNT] = {0};
  int64_t acc_n[KK_COUNT] = {0};
};

namespace {

void dense_stream_release(ife_ctx *ctx);  // dense_capi.inc

int fail(ife_ctx *ctx, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  else g_create_error = buf;
  return code;
}

#define IFE_HIP(ctx, call)                                                                  \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, e_ == hipErrorOutOfMemory ? IFE_E_NOMEM : IFE_E_HIP, "%s: %s", #call, \
                  hipGetErrorString(e_));                                                   \
  } while (0)

int ensure(ife_ctx *ctx, DevBuf &b, size_t bytes) {
  if (b.cap >= bytes) return IFE_OK;
  if (b.p) IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  IFE_HIP(ctx, b.grow(bytes));
  return IFE_OK;
}

int check_vol(ife_ctx *ctx, const ife_volume_desc *v, bool need_iir) {
  if (!v) return fail(ctx, IFE_E_ARG, "volume descriptor is null");
  if (v->nx <= 0 || v->ny <= 0 || v->nz <= 0)
    return fail(ctx, IFE_E_SIZE, "volume size must be positive (got %lld x %lld x %lld)",
                (long long)v->nx, (long long)v->ny, (long long)v->nz);
  if (v->nx > 0x7fffffff || v->ny > 0x7fffffff || v->nz > 0x7fffffff)
    return fail(ctx, IFE_E_SIZE, "axis length exceeds 2^31-1");
  if (!(v->sx > 0.0) || !(v->sy > 0.0) || !(v->sz > 0.0))
    return fail(ctx, IFE_E_ARG, "spacing must be positive");
  if (need_iir && (v->nx < 4 || v->ny < 4 || v->nz < 4))
    return fail(ctx, IFE_E_SIZE,
                "the recursive Gaussian needs at least 4 voxels along every axis "
                "(got %lld x %lld x %lld)",
                (long long)v->nx, (long long)v->ny, (long long)v->nz);
  return IFE_OK;
}

// ---- profiling -------------------------------------------------------------------
struct ProfScope {
  ife_ctx *ctx;
  ProfRec rec;
  bool on;
  ProfScope(ife_ctx *c, int kind) : ctx(c), on(c->profile != 0) {
    if (!on) return;
    rec.kind = kind;
    auto get = [&]() {
      hipEvent_t e;
      if (!ctx->ev_pool.empty()) {
        e = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
      } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
      }
      return e;
    };
    rec.a = get();
    rec.b = get();
    if (!rec.a || !rec.b) { on = false; return; }
    (void)hipEventRecord(rec.a, ctx->stream);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(rec.b, ctx->stream);
    ctx->prof.push_back(rec);
  }
};

int drain_profile(ife_ctx *ctx) {
  if (ctx->prof.empty()) return IFE_OK;
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (auto &r : ctx->prof) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      ctx->acc_ms[r.kind] += ms;
      ctx->acc_n[r.kind] += 1;
    }
    ctx->ev_pool.push_back(r.a);
    ctx->ev_pool.push_back(r.b);
  }
  ctx->prof.clear();
  return IFE_OK;
}

// ---- recursive Gaussian coefficients ------------------------------------------------
// [ITK-upstream] itk::RecursiveGaussianImageFilter::SetUp, ZeroOrder,
// NormalizeAcrossScale off.  Host-side, double.
// sin and cos of the pole angles through ONE sincos call, as GCC compiles ITK's adjacent
// std::sin / std::cos: glibc's sincos and cos differ in the last bit for some arguments, and
// 1 + sum(D) amplifies that to one float ulp of an output at one sample in 10^8-10^9
// (oracle/ife_oracle.c: pole_sincos; found by tests/test_gpu_fuzz.py).
void pole_sincos(double x, double &s, double &c) { ::sincos(x, &s, &c); }

// D from the poles (the same for every order).
void d_coefficients(double sd, double W1, double L1, double W2, double L2, IirCoef *c) {
  double Sin1, Sin2, Cos1, Cos2;
  pole_sincos(W1 / sd, Sin1, Cos1);
  pole_sincos(W2 / sd, Sin2, Cos2);
  (void)Sin1; (void)Sin2;
  const double Exp1 = std::exp(L1 / sd), Exp2 = std::exp(L2 / sd);
  c->D4 = Exp1 * Exp1 * Exp2 * Exp2;
  c->D3 = -2 * Cos1 * Exp1 * Exp2 * Exp2;
  c->D3 += -2 * Cos2 * Exp2 * Exp1 * Exp1;
  c->D2 = 4 * Cos2 * Cos1 * Exp1 * Exp2;
  c->D2 += Exp1 * Exp1 + Exp2 * Exp2;
  c->D1 = -2 * (Exp2 * Cos2 + Exp1 * Cos1);
}
// N of one term of the exponential series, with its sums SN, DN = sum(i N_i), EN = sum(i^2 N_i).
void n_coefficients(double sd, double A1, double B1, double W1, double L1, double A2, double B2,
                    double W2, double L2, double &N0, double &N1, double &N2, double &N3, double &SN,
                    double &DN, double &EN) {
  double Sin1, Sin2, Cos1, Cos2;
  pole_sincos(W1 / sd, Sin1, Cos1);
  pole_sincos(W2 / sd, Sin2, Cos2);
  const double Exp1 = std::exp(L1 / sd), Exp2 = std::exp(L2 / sd);
  N0 = A1 + A2;
  N1 = Exp2 * (B2 * Sin2 - (A2 + 2 * A1) * Cos2);
  N1 += Exp1 * (B1 * Sin1 - (A1 + 2 * A2) * Cos1);
  N2 = (A1 + A2) * Cos2 * Cos1;
  N2 -= B1 * Cos2 * Sin1 + B2 * Cos1 * Sin2;
  N2 *= 2 * Exp1 * Exp2;
  N2 += A2 * Exp1 * Exp1 + A1 * Exp2 * Exp2;
  N3 = Exp2 * Exp1 * Exp1 * (B2 * Sin2 - A2 * Cos2);
  N3 += Exp1 * Exp2 * Exp2 * (B1 * Sin1 - A1 * Cos1);
  SN = N0 + N1 + N2 + N3;
  DN = N1 + 2 * N2 + 3 * N3;
  EN = N1 + 4 * N2 + 9 * N3;
}
// M (anticausal) and the boundary coefficients from N and D; the first order is antisymmetric.
void m_and_boundary(IirCoef *c, bool symmetric) {
  if (symmetric) {
    c->M1 = c->N1 - c->D1 * c->N0; c->M2 = c->N2 - c->D2 * c->N0;
    c->M3 = c->N3 - c->D3 * c->N0; c->M4 = -c->D4 * c->N0;
  } else {
    c->M1 = -(c->N1 - c->D1 * c->N0); c->M2 = -(c->N2 - c->D2 * c->N0);
    c->M3 = -(c->N3 - c->D3 * c->N0); c->M4 = c->D4 * c->N0;
  }
  const double SN2 = c->N0 + c->N1 + c->N2 + c->N3;
  const double SM2 = c->M1 + c->M2 + c->M3 + c->M4;
  const double SD2 = 1.0 + c->D1 + c->D2 + c->D3 + c->D4;
  c->BN1 = c->D1 * SN2 / SD2; c->BN2 = c->D2 * SN2 / SD2;
  c->BN3 = c->D3 * SN2 / SD2; c->BN4 = c->D4 * SN2 / SD2;
  c->BM1 = c->D1 * SM2 / SD2; c->BM2 = c->D2 * SM2 / SD2;
  c->BM3 = c->D3 * SM2 / SD2; c->BM4 = c->D4 * SM2 / SD2;
}
// Order 0 is ITK's ZeroOrder case.  Orders 1 and 2 of the same routine (row f4; the reference
// only sketches their use, NormalizedGaussianConvolutionImageFilter.h:28-44): per-order constants
// of the exponential series, normalisation to a unit response on a unit ramp / unit parabola in
// pixel units, and the antisymmetric form of the anticausal coefficients for the first order.
int gauss_coeffs_order(double sigma, double spacing, int order, IirCoef *c) {
  const double A1[3] = {1.3530, -0.6724, -1.3563}, B1[3] = {1.8151, -3.4327, 5.2318};
  const double A2[3] = {-0.3531, 0.6724, 0.3446}, B2[3] = {0.0902, 0.6100, -2.2355};
  const double W1 = 0.6681, L1 = -1.3932, W2 = 2.0787, L2 = -1.3732;
  if (order < 0 || order > 2) return -1;
  double direction = 1.0;
  if (spacing < 0.0) { direction = -1.0; spacing = -spacing; }
  if (spacing < 1e-8) return -1;
  const double sd = sigma / spacing;
  d_coefficients(sd, W1, L1, W2, L2, c);
  const double SD = 1.0 + c->D1 + c->D2 + c->D3 + c->D4;
  const double DD = c->D1 + 2 * c->D2 + 3 * c->D3 + 4 * c->D4;
  const double ED = c->D1 + 4 * c->D2 + 9 * c->D3 + 16 * c->D4;
  if (order == 0) {
    double SN, DN, EN;
    n_coefficients(sd, A1[0], B1[0], W1, L1, A2[0], B2[0], W2, L2, c->N0, c->N1, c->N2, c->N3, SN, DN, EN);
    const double alpha0 = 2 * SN / SD - c->N0;
    const double nrm = 1.0 / alpha0;
    c->N0 *= nrm; c->N1 *= nrm; c->N2 *= nrm; c->N3 *= nrm;
  } else if (order == 1) {
    double SN, DN, EN;
    n_coefficients(sd, A1[1], B1[1], W1, L1, A2[1], B2[1], W2, L2, c->N0, c->N1, c->N2, c->N3, SN, DN, EN);
    double alpha1 = 2 * (SN * DD - DN * SD) / (SD * SD);
    alpha1 *= direction;
    c->N0 *= 1.0 / alpha1; c->N1 *= 1.0 / alpha1; c->N2 *= 1.0 / alpha1; c->N3 *= 1.0 / alpha1;
  } else {
    double N0_0, N1_0, N2_0, N3_0, N0_2, N1_2, N2_2, N3_2, SN0, DN0, EN0, SN2, DN2, EN2;
    n_coefficients(sd, A1[0], B1[0], W1, L1, A2[0], B2[0], W2, L2, N0_0, N1_0, N2_0, N3_0, SN0, DN0, EN0);
    n_coefficients(sd, A1[2], B1[2], W1, L1, A2[2], B2[2], W2, L2, N0_2, N1_2, N2_2, N3_2, SN2, DN2, EN2);
    const double beta = -(2 * SN2 - SD * N0_2) / (2 * SN0 - SD * N0_0);
    const double N0 = N0_2 + beta * N0_0, N1 = N1_2 + beta * N1_0;
    const double N2 = N2_2 + beta * N2_0, N3 = N3_2 + beta * N3_0;
    const double SN = SN2 + beta * SN0, DN = DN2 + beta * DN0, EN = EN2 + beta * EN0;
    const double alpha2 = (EN * SD * SD - ED * SN * SD - 2 * DN * DD * SD + 2 * DD * DD * SN) / (SD * SD * SD);
    c->N0 = N0 * (1.0 / alpha2); c->N1 = N1 * (1.0 / alpha2);
    c->N2 = N2 * (1.0 / alpha2); c->N3 = N3 * (1.0 / alpha2);
  }
  m_and_boundary(c, order != 1);
  return 0;
}

// Constant lines (IFE_OPT_CONST_LINES): what does the recursive Gaussian of this axis make of a
// line whose n samples all have the value xin?  Simulated here in the arithmetic of the line
// kernels -- the same double operations in the same order (this translation unit is built with
// -ffp-contract=off on both sides), signs of zero included -- so the answer found here holds
// there.  True when every output has the same bit pattern, returned in *resp.
// (Restates FilterDataArray like iir_kernels.inc, for one line.)
bool const_response(const IirCoef &c, int64_t n, double xin, float *resp) {
  if (n < 4 || n > 65536) return false;
  std::vector<double> ca((size_t)n);
  double x1 = xin, x2 = xin, x3 = xin, y1 = xin, y2 = xin, y3 = xin, y4 = xin;
  for (int64_t i = 0; i < n; ++i) {
    const double d1 = i < 1 ? c.BN1 : c.D1, d2 = i < 2 ? c.BN2 : c.D2;
    const double d3 = i < 3 ? c.BN3 : c.D3, d4 = i < 4 ? c.BN4 : c.D4;
    const double a = x3 * c.N3 + (x2 * c.N2 + (x1 * c.N1 + xin * c.N0));
    const double t = y4 * d4 + (y3 * d3 + (y2 * d2 + y1 * d1));
    const double y = a - t;
    x3 = x2; x2 = x1; x1 = xin;
    y4 = y3; y3 = y2; y2 = y1; y1 = y;
    ca[(size_t)i] = y;
  }
  double u1 = xin, u2 = xin, u3 = xin, u4 = xin;
  x1 = x2 = x3 = xin;
  double x4 = xin;
  uint32_t first = 0;
  for (int64_t i = n - 1; i >= 0; --i) {
    const double d1 = i + 1 >= n ? c.BM1 : c.D1, d2 = i + 2 >= n ? c.BM2 : c.D2;
    const double d3 = i + 3 >= n ? c.BM3 : c.D3, d4 = i + 4 >= n ? c.BM4 : c.D4;
    const double a = x4 * c.M4 + (x3 * c.M3 + (x2 * c.M2 + x1 * c.M1));
    const double t = u4 * d4 + (u3 * d3 + (u2 * d2 + u1 * d1));
    const double y = a - t;
    x4 = x3; x3 = x2; x2 = x1; x1 = xin;
    u4 = u3; u3 = u2; u2 = u1; u1 = y;
    const float o = (float)(ca[(size_t)i] + y);
    uint32_t bits;
    memcpy(&bits, &o, 4);
    if (i == n - 1) first = bits;
    else if (bits != first) return false;
  }
  memcpy(resp, &first, 4);
  return true;
}
// IirJob::const_lines for one job: bit 0: a line of +0 comes out as +0; bit 1: a line of 1.0f as
// 1.0f; bit 2 / bit 3: a line of -0 comes out as -0 / as +0 (T * 0 is -0 wherever T < 0, so the
// exterior of a CT numerator is made of such lines).  Anything else is filtered.
uint32_t const_line_flags(const IirCoef &c, int64_t n) {
  uint32_t f = 0, bits;
  float r;
  if (const_response(c, n, 0.0, &r)) { memcpy(&bits, &r, 4); if (bits == 0u) f |= 1u; }
  if (const_response(c, n, 1.0, &r) && r == 1.0f) f |= 2u;
  if (const_response(c, n, -0.0, &r)) {
    memcpy(&bits, &r, 4);
    if (bits == 0x80000000u) f |= 4u;
    else if (bits == 0u) f |= 8u;
  }
  return f;
}

// [ITK-upstream] DerivativeOperator coefficients after FlipAxes + ScaleCoefficients:
// order 1 -> {-0.5, 0, 0.5} * s ; order 2 -> {1, -2, 1} * s  (s = 1/spacing, or
// 1/spacing^2 for order 2 with IFE_OPT_DSCALE_MODE=1).
DerivCoef deriv_coeffs(const ife_volume_desc *v, int dscale_mode) {
  DerivCoef d;
  const double sp[3] = {v->sx, v->sy, v->sz};
  for (int a = 0; a < 3; ++a) {
    const double s1 = 1.0 / sp[a];
    const double s2 = dscale_mode == 1 ? s1 * s1 : s1;
    d.m1[a] = -0.5 * s1;
    d.p1[a] = 0.5 * s1;
    d.a2[a] = 1.0 * s2;
    d.b2[a] = -2.0 * s2;
    d.c2[a] = 1.0 * s2;
  }
  return d;
}

IirGeom geom_for_axis(const ife_volume_desc *v, int axis) {
  IirGeom g;
  g.in_w = 0; g.in_group = 0; g.in_nz = 0;
  const int64_t nx = v->nx, ny = v->ny, nz = v->nz;
  if (axis == 2) {
    g.n = nz; g.nlines = nx * ny; g.sstride = nx * ny; g.inner = nx * ny; g.outer = 0;
  } else if (axis == 1) {
    g.n = ny; g.nlines = nx * nz; g.sstride = nx; g.inner = nx; g.outer = nx * ny;
  } else {
    g.n = nx; g.nlines = ny * nz; g.sstride = 1; g.inner = 1; g.outer = nx;
  }
  return g;
}

// checkpoint slots per line: one per register block covers both granularities
size_t ck_pairs(int64_t n, int K) { return (size_t)((n + K - 1) / K); }

int ensure_ck(ife_ctx *ctx, const ife_volume_desc *v, int njobs) {
  const int K = 8;  // sized for the smallest register block any axis may run with
  size_t need_y = 0;
  for (int a = 0; a < 3; ++a) {
    IirGeom g = geom_for_axis(v, a);
    const size_t np = ck_pairs(g.n, K);
    need_y = std::max(need_y, np * 4 * (size_t)g.nlines * sizeof(double));
  }
  for (int j = 0; j < njobs; ++j) {
    int rc = ensure(ctx, ctx->ck_y[j], need_y);
    if (rc) return rc;
  }
  return IFE_OK;
}

int ensure_slots(ife_ctx *ctx, const ife_volume_desc *v, int nslots) {
  const size_t nb = (size_t)(v->nx * v->ny * v->nz) * sizeof(float);
  for (int s = 0; s < nslots; ++s)
    for (int i = 0; i < 4; ++i) {
      int rc = ensure(ctx, ctx->fld[s][i], nb);
      if (rc) return rc;
    }
  return IFE_OK;
}

// One launch of the line kernel along `axis` over njobs independent float volumes
// (jobs = numerator / denominator of up to three scales), each with its own sigma.
// `in2` (strided axes, pair checkpoints only): jobs are PAIRED -- in[j] numerator, in2[j]
// denominator, out[j] their quotient; job j uses checkpoint areas j and njobs + j.
// `zs` (Z axis, pair checkpoints; jobs ordered scale-major, zs->nf fields per scale): the causal
// sweeps of all jobs run first as ONE launch from the raw image and mask (iir_sweep_z_kernel,
// which also leaves the sources in[] point at, unless !zs->write_src), and the line kernel
// proper runs in its backward-only form.
struct ZSweepSrc {
  const void *img, *msk;  // msk null: no mask, one field
  int img_dtype, msk_dtype;
  float *tc, *cf;
  int nf;
  bool write_src;
};
int launch_iir(ife_ctx *ctx, const ife_volume_desc *v, int axis, int njobs,
               const float *const *in, float *const *out, const double *sigma,
               int in_y_chunks = 1, const int *order = nullptr /* per job: 0 (default), 1, 2 */,
               const float *const *in2 = nullptr, const ZSweepSrc *zs = nullptr) {
  if (njobs < 1 || njobs > IIR_MAX_JOBS) return fail(ctx, IFE_E_ARG, "bad job count %d", njobs);
  IirGeom g = geom_for_axis(v, axis);
  if (in_y_chunks > 1) {
    if (axis != 0) return fail(ctx, IFE_E_ARG, "Y-chunked input is only read by the x pass");
    if (v->ny % in_y_chunks || (v->ny / in_y_chunks) % 64)
      return fail(ctx, IFE_E_SIZE, "Y-chunked input needs ny/chunks to be a multiple of 64");
    g.in_w = in_y_chunks;
    g.in_group = v->ny / in_y_chunks;
    g.in_nz = v->nz;
  }
  // 32-bit offsets of the buffer accesses (iir_kernels.inc "addressing")
  if ((int64_t)2 * 16 * g.sstride * 4 >= (int64_t)1 << 31 ||
      g.outer * 4 >= (int64_t)1 << 32 || g.nlines * 8 * 3 >= (int64_t)1 << 32)
    return fail(ctx, IFE_E_SIZE, "volume too large for the 32-bit offsets of the line kernels");
  if (in2 && (axis == 0 || 2 * njobs > IIR_MAX_JOBS || ctx->iir_ckpt != 2))
    return fail(ctx, IFE_E_ARG, "the paired form runs on the strided axes with at most %d jobs", IIR_MAX_JOBS / 2);
  if (zs && (axis != 2 || in2 || order || ctx->iir_ckpt != 2 || zs->nf < 1 || zs->nf > 2 || njobs % zs->nf ||
             njobs / zs->nf > IFE_MAX_SLOTS || !zs->img || !zs->tc || (zs->nf == 2 && (!zs->msk || !zs->cf))))
    return fail(ctx, IFE_E_ARG, "the shared sweep runs the Z pass of up to %d scales with pair checkpoints", IFE_MAX_SLOTS);
  int rc = ensure_ck(ctx, v, in2 ? 2 * njobs : njobs);
  if (rc) return rc;
  if (zs && (rc = ensure(ctx, ctx->zs_rec, (size_t)zs->nf * (size_t)g.nlines * sizeof(uint32_t)))) return rc;
  uint32_t any_const = 0;
  const double sp = axis == 0 ? v->sx : axis == 1 ? v->sy : v->sz;
  IirJobs jobs;
  memset(&jobs, 0, sizeof jobs);
  for (int j = 0; j < njobs; ++j) {
    if (!in[j] || !out[j] || in[j] == out[j]) return fail(ctx, IFE_E_ARG, "bad job buffers");
    if ((reinterpret_cast<uintptr_t>(in[j]) | reinterpret_cast<uintptr_t>(out[j])) % 4)
      return fail(ctx, IFE_E_ARG, "field pointers must be aligned to 4 bytes");
    jobs.j[j].in = in[j];
    jobs.j[j].out = out[j];
    jobs.j[j].ck_y = (double *)ctx->ck_y[j].p;
    if (in2) {
      if (!in2[j] || in2[j] == out[j] || reinterpret_cast<uintptr_t>(in2[j]) % 4)
        return fail(ctx, IFE_E_ARG, "bad denominator buffer");
      jobs.j[j].in2 = in2[j];
      jobs.j[j].ck_y2 = (double *)ctx->ck_y[njobs + j].p;
    }
    if (gauss_coeffs_order(sigma[j], sp, order ? order[j] : 0, &jobs.j[j].c))
      return fail(ctx, IFE_E_ARG, "spacing is suspiciously small");
    // constant lines are copied where this filter provably maps the constant to a constant
    // (const_line_flags: simulated on the host for these coefficients and this line length,
    // remembered per context; zero-order only)
    jobs.j[j].const_lines = 0;
    if (ctx->const_lines && !ctx->iir_fma && (!order || order[j] == 0)) {
      const int64_t len = axis == 0 ? v->nx : axis == 1 ? v->ny : v->nz;
      const std::tuple<double, double, int64_t> key(sigma[j], sp, len);
      auto it = ctx->const_flags.find(key);
      if (it == ctx->const_flags.end()) {
        if (ctx->const_flags.size() > 256) ctx->const_flags.clear();
        it = ctx->const_flags.emplace(key, const_line_flags(jobs.j[j].c, len)).first;
      }
      jobs.j[j].const_lines = it->second;
    }
    any_const |= jobs.j[j].const_lines;
    if (zs) jobs.j[j].line_rec = (const uint32_t *)ctx->zs_rec.p + (size_t)(j % zs->nf) * (size_t)g.nlines;
  }
  g.njobs = njobs;
  g.ngroups = (int32_t)((g.nlines + (in2 ? 127 : 255)) / (in2 ? 128 : 256));  // paired: 128 lines x 2 fields
  const dim3 grid((unsigned)((g.ngroups + 7) / 8 * 8 * njobs), 1, 1);  // job-fastest, padded
  const int sblock = ctx->iir_block ? ctx->iir_block : 12;
  if (zs) {
    // booked as `prep`: it stands where the prepass stood (13 B of sources per voxel) and one
    // iir_z launch per step follows, as before
    ProfScope pz(ctx, KK_PREP);
    ZSweepArgs za;
    za.img = zs->img; za.msk = zs->msk; za.tc = zs->tc; za.cf = zs->cf;
    za.rec = (uint32_t *)ctx->zs_rec.p;
    za.nf = zs->nf; za.write_src = zs->write_src ? 1 : 0; za.track = any_const ? 1 : 0;
    IirGeom gs = g;
    gs.njobs = zs->nf;  // workgroups: field-fastest within a run of eight line groups
    const dim3 sgrid((unsigned)((gs.ngroups + 7) / 8 * 8 * zs->nf), 1, 1);
    with_iir_kernels(ctx->iir_fma, [&](auto ks) {
      using KS = decltype(ks);
      with_const<8, 10, 12, 16>(sblock, [&](auto K) {
        with_const<1, 2, 3>(njobs / zs->nf, [&](auto S) {
          auto launch = [&](auto ti, auto tm) {
            hipLaunchKernelGGL((KS::template sweep_z<decltype(K)::value, decltype(S)::value, decltype(ti), decltype(tm)>),
                               sgrid, dim3(256), 0, ctx->stream, jobs, gs, za);
          };
          auto with_mask = [&](auto ti) {
            if (zs->msk && zs->msk_dtype == IFE_U16) launch(ti, uint16_t{});
            else launch(ti, uint8_t{});
          };
          if (zs->img_dtype == IFE_F32) with_mask(float{});
          else with_mask(int16_t{});
        });
      });
    });
    IFE_HIP(ctx, hipGetLastError());
  }
  ProfScope ps(ctx, axis == 2 ? KK_IIR_Z : axis == 1 ? KK_IIR_Y : KK_IIR_X);
  // register block of the strided axes: 12 for both (three waves per SIMD, 2.7 B of checkpoints
  // per sample).  Round 2 ran z with blocks of 10 for a fourth wave per SIMD; since the waits
  // are exact (iir_kernels.inc "Memory operations and waits") three waves hide the latency and
  // the fewer checkpoints win: z 1.85 -> 1.74 ms, y 1.87 with 12 against 2.06 with 16.
  with_iir_kernels(ctx->iir_fma, [&](auto ks) {
    using KS = decltype(ks);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, jobs, g); };
    if (zs)
      with_const<8, 10, 12, 16>(sblock, [&](auto K) { launch(KS::template strided<decltype(K)::value, false, true>); });
    else if (in2)
      with_const<8, 10, 12, 16>(sblock, [&](auto K) { launch(KS::template strided<decltype(K)::value, true, false>); });
    else if (axis == 0)
      with_const<8, 16>(ctx->iir_block, [&](auto K) { launch(KS::template contig<decltype(K)::value>); });
    else if (ctx->iir_ckpt == 1)
      with_const<8, 16>(ctx->iir_block, [&](auto K) { launch(KS::template strided1<decltype(K)::value>); });
    else
      with_const<8, 10, 12, 16>(sblock, [&](auto K) { launch(KS::template strided<decltype(K)::value, false, false>); });
  });
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

// ---- Z pass of a Z-slab (iir_types.hpp "ZSlabJob") -----------------------------------
#ifndef IFE_ZSLAB_K
#define IFE_ZSLAB_K 12
#endif
constexpr int ZSLAB_K = IFE_ZSLAB_K;  // register block of the slab kernels (fixes the checkpoint layout)
int64_t zslab_pairs(int64_t n) { return ((n + ZSLAB_K - 1) / ZSLAB_K + 1) / 2; }
size_t zslab_ck_bytes(const ife_volume_desc *v) {
  const size_t L = (size_t)(v->nx * v->ny);
  return (size_t)zslab_pairs(v->nz) * 4 * L * 2 * sizeof(double);
}
// phase 0: causal sweep, 1: anticausal sweep, 2: combine, 3 / 4: fused with the causal /
// anticausal recursion carried through the slab (zslab_fused_kernel).  orders: per job 0, 1 or 2
// (null: all zero).  A lean sweep (phase 0 / 1) runs every three consecutive jobs with the same
// input, the same sigma and the orders 0, 1, 2 through the shared-read kernels (zslab_causal3 /
// zslab_anti3_kernel: one load per plane for the three), every other job through the per-job one.
int launch_zslab(ife_ctx *ctx, int phase, int njobs, const float *const *in, float *const *out,
                 const ife_volume_desc *v, int64_t line0, int64_t nlines, const double *sigmas,
                 int has_lo, int has_hi, const void *state_in, void *state_out, void *const *ck,
                 const int *orders = nullptr) {
  if (njobs < 1 || njobs > IIR_MAX_JOBS) return fail(ctx, IFE_E_ARG, "bad job count %d", njobs);
  for (int j = 0; orders && j < njobs; ++j)
    if (orders[j] < 0 || orders[j] > 2)
      return fail(ctx, IFE_E_ARG, "the order of the recursive Gaussian must be 0, 1 or 2");
  const int64_t L = v->nx * v->ny, n = v->nz;
  if (line0 < 0 || nlines < 1 || line0 + nlines > L)
    return fail(ctx, IFE_E_ARG, "line range [%lld, %lld) outside the %lld lines of the slab",
                (long long)line0, (long long)(line0 + nlines), (long long)L);
  if (n < 4) return fail(ctx, IFE_E_SIZE, "a Z-slab needs at least 4 planes (got %lld)", (long long)n);
  // 32-bit offsets of the buffer accesses (iir_kernels.inc "addressing")
  if ((int64_t)2 * ZSLAB_K * L * 4 >= (int64_t)1 << 31 || L * 8 * 3 >= (int64_t)1 << 32)
    return fail(ctx, IFE_E_SIZE, "slab too large for the 32-bit offsets of the line kernels");
  if (!in || !sigmas || !ck) return fail(ctx, IFE_E_ARG, "null pointer");
  const bool need_in = (phase == 0 || phase == 3) ? has_lo != 0 : (phase == 1 || phase == 4) ? has_hi != 0 : false;
  if ((phase != 2 && !state_out) || (need_in && !state_in)) return fail(ctx, IFE_E_ARG, "null state buffer");
  if ((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) % 8)
    return fail(ctx, IFE_E_ARG, "state buffers must be aligned to 8 bytes");
  const int64_t np = zslab_pairs(n);
  ZSlabJobs jobs, jobs3;  // per job; three by three for the shared-read sweeps
  memset(&jobs, 0, sizeof jobs);
  memset(&jobs3, 0, sizeof jobs3);
  int n1 = 0, n3 = 0, left3 = 0;  // jobs of `jobs`, sources of `jobs3`, jobs still to join the open three
  for (int j = 0; j < njobs; ++j) {
    if (left3 == 0 && phase < 2 && orders && j + 2 < njobs && in[j] == in[j + 1] && in[j] == in[j + 2] &&
        sigmas[j] == sigmas[j + 1] && sigmas[j] == sigmas[j + 2] && orders[j] == 0 && orders[j + 1] == 1 &&
        orders[j + 2] == 2)
      left3 = 3;
    ZSlabJob &J = left3 > 0 ? jobs3.j[3 * n3 + (3 - left3)] : jobs.j[n1++];
    if (left3 > 0 && --left3 == 0) ++n3;
    if (!in[j] || !ck[j] || (phase >= 2 && (!out || !out[j] || out[j] == in[j])))
      return fail(ctx, IFE_E_ARG, "bad job buffers");
    if (reinterpret_cast<uintptr_t>(ck[j]) % 8 || reinterpret_cast<uintptr_t>(in[j]) % 4)
      return fail(ctx, IFE_E_ARG, "job buffers are misaligned");
    J.in = in[j] + line0;
    J.out = phase >= 2 ? out[j] + line0 : nullptr;
    double *cy = (double *)ck[j];
    double *ay = cy + np * 4 * L;
    J.cy = cy + line0; J.ay = ay + line0;
    const size_t rec = (size_t)nlines * IFE_Z_STATE_BYTES;  // [4][nlines] doubles per job
    if (state_in) J.sin_y = (const double *)((const char *)state_in + (size_t)j * rec);
    if (state_out) J.sout_y = (double *)((char *)state_out + (size_t)j * rec);
    if (!(sigmas[j] > 0.0) || gauss_coeffs_order(sigmas[j], v->sz, orders ? orders[j] : 0, &J.c))
      return fail(ctx, IFE_E_ARG, "bad sigma or spacing");
  }
  // the shared-read kernels keep one set of feedback coefficients: they are a function of sigma
  // and spacing alone (gauss_coeffs_order)
  for (int t = 0; t < n3; ++t)
    for (int k = 1; k < 3; ++k)
      if (memcmp(&jobs3.j[3 * t].c.D1, &jobs3.j[3 * t + k].c.D1, 4 * sizeof(double)))
        return fail(ctx, IFE_E_STATE, "the feedback coefficients of one sigma differ between the orders");
  ZSlabGeom g;
  g.n = n; g.nlines = nlines; g.sstride = L; g.ck_stride = L;
  g.has_lo = has_lo ? 1 : 0; g.has_hi = has_hi ? 1 : 0;
  g.ngroups = (int32_t)((nlines + 255) / 256);
  ProfScope ps(ctx, phase >= 2 ? KK_ZSLAB_COMBINE : KK_ZSLAB_SWEEP);
  with_iir_kernels(ctx->iir_fma, [&](auto ks) {
    using KS = decltype(ks);
    auto launch = [&](auto kernel, const ZSlabJobs &js, int nj) {  // nj: what iir_block_of deals out
      if (nj == 0) return;
      g.njobs = nj;
      const dim3 grid((unsigned)((g.ngroups + 7) / 8 * 8 * nj), 1, 1);
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, js, g);
    };
    if (phase == 0) {
      launch(KS::template zslab_causal3<ZSLAB_K>, jobs3, n3);
      launch(KS::template zslab_causal<ZSLAB_K>, jobs, n1);
    } else if (phase == 1) {
      launch(KS::template zslab_anti3<ZSLAB_K>, jobs3, n3);
      launch(KS::template zslab_anti<ZSLAB_K>, jobs, n1);
    } else if (phase == 3) launch(KS::template zslab_fused<ZSLAB_K, 0>, jobs, n1);
    else if (phase == 4) launch(KS::template zslab_fused<ZSLAB_K, 1>, jobs, n1);
    else launch(KS::template zslab_combine<ZSLAB_K>, jobs, n1);
  });
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

template <typename TI, typename TM>
int launch_prep(ife_ctx *ctx, const TI *img, const TM *msk, float *tc, float *cf, int64_t n,
                PrepGeom pg = PrepGeom{0, 0, 0, 0, 0}) {
  ProfScope ps(ctx, KK_PREP);
  const uintptr_t al = reinterpret_cast<uintptr_t>(img) % (4 * sizeof(TI)) |
                       reinterpret_cast<uintptr_t>(msk) % (4 * sizeof(TM)) |
                       reinterpret_cast<uintptr_t>(tc) % 16 | reinterpret_cast<uintptr_t>(cf) % 16;
  const bool vec = al == 0 && (pg.chunks <= 1 || pg.nx % 4 == 0);
  const int64_t n4 = vec ? n / 4 : 0;
  if (n4 > 0) {
    // one 16-byte piece per thread (the kernel's loop runs once): on MI355X a stream moves
    // faster as many short-lived workgroups than as a grid-stride loop of a few thousand
    // (scripts/experiments/stream_probe.hip: fill 6.9 vs 5.0 TB/s, copy 6.4 vs 4.9)
    const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 0x7fffffff);
    hipLaunchKernelGGL((prep_kernel_vec4<TI, TM>), dim3(blocks), dim3(256), 0, ctx->stream, img,
                       msk, tc, cf, n4, pg);
    IFE_HIP(ctx, hipGetLastError());
  }
  if (n4 * 4 < n) {
    const int64_t rest = n - n4 * 4;
    const unsigned blocks = (unsigned)std::min<int64_t>((rest + 255) / 256, 8192);
    hipLaunchKernelGGL((prep_kernel_scalar<TI, TM>), dim3(blocks), dim3(256), 0, ctx->stream,
                       img, msk, tc, cf, n4 * 4, n, pg);
    IFE_HIP(ctx, hipGetLastError());
  }
  return IFE_OK;
}

// SmoothingRecursiveGaussianImageFilter for a group of up to IFE_MAX_SLOTS scales at
// once: Z pass from the shared sources (image*certainty, certainty), then X, then Y, each
// axis as ONE launch over all (scale, field) jobs.  Scale k of the group ends in slot k:
// numerator in fld[k][0], denominator in fld[k][2].
int smooth_group(ife_ctx *ctx, const float *src_num, const float *src_den,
                 const ife_volume_desc *v, const double *sigmas, int nscales, const ZSweepSrc *zs = nullptr) {
  const int nf = src_den ? 2 : 1;
  const float *in[IIR_MAX_JOBS];
  float *out[IIR_MAX_JOBS];
  double sg[IIR_MAX_JOBS];
  int nj = 0;
  for (int k = 0; k < nscales; ++k)
    for (int f = 0; f < nf; ++f) sg[nj++] = sigmas[k];
  int rc = ensure_slots(ctx, v, nscales);
  if (rc) return rc;
  auto fill = [&](int src_idx, int dst_idx, bool from_source) {
    int j = 0;
    for (int k = 0; k < nscales; ++k)
      for (int f = 0; f < nf; ++f, ++j) {
        in[j] = from_source ? (f == 0 ? src_num : src_den)
                            : (const float *)ctx->fld[k][2 * f + src_idx].p;
        out[j] = (float *)ctx->fld[k][2 * f + dst_idx].p;
      }
  };
  fill(0, 0, true);                                    // Z: sources -> ping
  rc = launch_iir(ctx, v, 2, nj, in, out, sg, 1, nullptr, nullptr, zs);
  fill(0, 1, false);                                   // X: ping -> pong
  if (!rc) rc = launch_iir(ctx, v, 0, nj, in, out, sg);
  if (nf == 2 && ctx->fused_divide && ctx->iir_ckpt == 2) {
    // Y: numerator and denominator in sibling waves, the quotient S goes to the numerator's slot
    const float *n1[IIR_MAX_JOBS], *d1[IIR_MAX_JOBS];
    float *o1[IIR_MAX_JOBS];
    double s1[IIR_MAX_JOBS];
    for (int k = 0; k < nscales; ++k) {
      n1[k] = (const float *)ctx->fld[k][1].p;
      d1[k] = (const float *)ctx->fld[k][3].p;
      o1[k] = (float *)ctx->fld[k][0].p;
      s1[k] = sigmas[k];
    }
    if (!rc) rc = launch_iir(ctx, v, 1, nscales, n1, o1, s1, 1, nullptr, d1);
    return rc;
  }
  fill(1, 0, false);                                   // Y: pong -> ping
  if (!rc) rc = launch_iir(ctx, v, 1, nj, in, out, sg);
  return rc;
}
// Everything smooth_group and the finite-difference scale loop allocate for this volume, now.
int reserve_smooth(ife_ctx *ctx, const ife_volume_desc *vol) {
  const size_t nb = (size_t)(vol->nx * vol->ny * vol->nz) * sizeof(float);
  int rc = ensure_slots(ctx, vol, IFE_MAX_SLOTS);
  for (int i = 0; i < 2 && !rc; ++i) rc = ensure(ctx, ctx->pre[i], nb);
  if (!rc) rc = ensure_ck(ctx, vol, 2 * IFE_MAX_SLOTS);
  return rc;
}
// After smooth_group: is slot k's fld[k][0] already the quotient S (denominator folded in)?
bool slots_hold_quotient(const ife_ctx *ctx, bool has_den) {
  return has_den && ctx->fused_divide && ctx->iir_ckpt == 2;
}

// Vector loads and stores: a misaligned pointer would fault on the device, so it is refused on the
// host (include/ife_hip.h, IFE_MEM_DEVICE: inputs to their element size, interleaved outputs of
// eight components to 16 bytes, of six or ten to 8).  b may be null.
int check_in_alignment(ife_ctx *ctx, const void *a, size_t a_size, const void *b, size_t b_size) {
  if (reinterpret_cast<uintptr_t>(a) % a_size || (b && reinterpret_cast<uintptr_t>(b) % b_size))
    return fail(ctx, IFE_E_ARG, "input pointers must be aligned to their element size");
  return IFE_OK;
}
int check_out_alignment(ife_ctx *ctx, const void *out, int nout, int layout) {
  const uintptr_t need = layout == IFE_PLANAR ? 4 : (nout == 8 ? 16 : nout % 2 == 0 ? 8 : 4);
  if (reinterpret_cast<uintptr_t>(out) % need)
    return fail(ctx, IFE_E_ARG, "output pointer must be aligned to %d bytes for this layout", (int)need);
  return IFE_OK;
}

template <int MODE, typename VAL, typename TM>
int launch_features(ife_ctx *ctx, VAL val, const TM *mask, float *out,
                    const ife_volume_desc *v, int layout, int halo_lo = 0, int halo_hi = 0,
                    const uint32_t *seg_base = nullptr, int64_t col_stride = 0,
                    int64_t col_offset = 0) {
  if constexpr (std::is_same<VAL, ValSmooth>::value) {
    // no denominator (certainty identically one): the single-field source, a kernel without
    // the run-time choice (measured 1.39 -> 1.23 ms per launch at 512^3)
    if (val.den == nullptr)
      return launch_features<MODE>(ctx, ValS{val.num}, mask, out, v, layout, halo_lo, halo_hi,
                                   seg_base, col_stride, col_offset);
  }
  FeatGeom g;
  g.seg_base = seg_base;
  g.col_offset = col_offset;
  g.nx = (int)v->nx; g.ny = (int)v->ny; g.nz = (int)v->nz;
  g.zchunk = ctx->zchunk;
  g.plane = v->nx * v->ny;
  g.nvox = MODE == FEAT_SAMPLES8 ? col_stride : g.plane * v->nz;
  g.zoff = halo_lo ? 1 : 0;
  g.zc_hi = (int)v->nz + g.zoff + (halo_hi ? 1 : 0) - 1;
  const DerivCoef dc = deriv_coeffs(v, ctx->dscale_mode);
  g.gx = (int)((v->nx + FT_TX - 1) / FT_TX);
  g.gy = (int)((v->ny + FT_TY - 1) / FT_TY);
  g.gz = (int)((v->nz + g.zchunk - 1) / g.zchunk);
  const int64_t nblocks = (int64_t)g.gx * g.gy * g.gz;
  if (nblocks > 0x7fffffff) return fail(ctx, IFE_E_SIZE, "volume too large for the feature kernel grid");
  if (int rc = check_out_alignment(ctx, out, FeatNOut<MODE>::value, layout)) return rc;
  dim3 grid((unsigned)nblocks, 1, 1);
  ProfScope ps(ctx, KK_FEATURES);
  const bool unit = v->sx == 1.0 && v->sy == 1.0 && v->sz == 1.0;
  const int planar = layout == IFE_PLANAR ? 1 : 0;
  constexpr bool has_eig = MODE == FEAT_FEATURES8 || MODE == FEAT_EIG6 || MODE == FEAT_SAMPLES8;
  // ring form (feature_kernels.hpp): one float field, narrow mask, dword-aligned mask planes,
  // in-plane byte offsets that fit 32 bits
  constexpr bool ring_types = (std::is_same<VAL, ValS>::value || std::is_same<VAL, ValRaw<float>>::value) &&
                              sizeof(TM) <= 2;
  bool ring = false;
  const float *ring_src = nullptr;
  if constexpr (ring_types) {
    if constexpr (std::is_same<VAL, ValS>::value) ring_src = val.s;
    else ring_src = val.img;
    const int64_t row_bytes = v->nx * (int64_t)sizeof(TM), plane_bytes = g.plane * (int64_t)sizeof(TM);
    ring = ctx->feat_ring && g.plane < ((int64_t)1 << 30) && reinterpret_cast<uintptr_t>(ring_src) % 4 == 0 &&
           (mask == nullptr ||
            (row_bytes % 4 == 0 && plane_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0));
  }
  auto launch = [&](auto UNIT, auto TRIG, auto PL) {
    constexpr bool U = decltype(UNIT)::value != 0, P = decltype(PL)::value != 0;
    constexpr int T = decltype(TRIG)::value;
    if constexpr (ring_types) {
      if (ring) {
        hipLaunchKernelGGL((features_ring_kernel<MODE, U, T, P, TM>), grid, dim3(FT_THREADS), 0, ctx->stream,
                           ring_src, mask, out, g, dc);
        return;
      }
    }
    hipLaunchKernelGGL((features_kernel<MODE, U, T, P, VAL, TM>), grid, dim3(FT_THREADS), 0, ctx->stream, val,
                       mask, out, g, dc);
  };
  // unit spacing, then the trigonometry (only kernels with eigenvalues have one to choose), then
  // the layout (the sample columns are planar by construction)
  with_const<1, 0>(unit, [&](auto UNIT) {
    auto with_trig = [&](auto TRIG) {
      if constexpr (MODE == FEAT_SAMPLES8) launch(UNIT, TRIG, std::true_type{});
      else with_const<1, 0>(planar, [&](auto PL) { launch(UNIT, TRIG, PL); });
    };
    if constexpr (has_eig) with_const<1, 2, 0>(ctx->trig_mode, with_trig);
    else with_trig(std::integral_constant<int, 0>{});
  });
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

size_t dtype_size(int dt) {
  switch (dt) {
    case IFE_F32: return 4;
    case IFE_I16: return 2;
    case IFE_U8: return 1;
    case IFE_U16: return 2;
  }
  return 0;
}

// ---- argument checks shared by the entry points (status returned, message through fail) ----
int check_mem(ife_ctx *ctx, int mem) {
  if (mem != IFE_MEM_HOST && mem != IFE_MEM_DEVICE) return fail(ctx, IFE_E_ARG, "bad mem %d", mem);
  return IFE_OK;
}
int check_layout_mem(ife_ctx *ctx, int layout, int mem) {
  if (layout != IFE_INTERLEAVED && layout != IFE_PLANAR)
    return fail(ctx, IFE_E_ARG, "bad layout %d", layout);
  return check_mem(ctx, mem);
}
int check_image_dtype(ife_ctx *ctx, int dt) {
  if (dt != IFE_F32 && dt != IFE_I16) return fail(ctx, IFE_E_ARG, "image dtype must be IFE_F32 or IFE_I16");
  return IFE_OK;
}
// a null mask (certainty one everywhere) passes with any dtype where may_be_null
int check_mask_dtype(ife_ctx *ctx, const void *mask, int dt, bool may_be_null) {
  if (!mask) return may_be_null ? IFE_OK : fail(ctx, IFE_E_ARG, "null pointer");
  if (dt != IFE_U8 && dt != IFE_U16) return fail(ctx, IFE_E_ARG, "mask dtype must be IFE_U8 or IFE_U16");
  return IFE_OK;
}
int check_sigma(ife_ctx *ctx, double sigma) {
  if (!(sigma > 0.0)) return fail(ctx, IFE_E_ARG, "sigma must be positive");
  return IFE_OK;
}
int check_sigmas(ife_ctx *ctx, const float *sigmas, int n_sigmas) {
  if (n_sigmas < 1) return fail(ctx, IFE_E_ARG, "at least one sigma is required");
  for (int s = 0; s < n_sigmas; ++s)
    if (!(sigmas[s] > 0.0f)) return fail(ctx, IFE_E_ARG, "sigma[%d] must be positive", s);
  return IFE_OK;
}
int check_axis(ife_ctx *ctx, int axis) {
  if (axis < 0 || axis > 2) return fail(ctx, IFE_E_ARG, "axis must be 0 (x), 1 (y) or 2 (z)");
  return IFE_OK;
}
int check_axis_len(ife_ctx *ctx, const ife_volume_desc *v, int axis) {
  if ((axis == 0 ? v->nx : axis == 1 ? v->ny : v->nz) < 4)
    return fail(ctx, IFE_E_SIZE, "the recursive Gaussian needs at least 4 voxels along axis %d", axis);
  return IFE_OK;
}

// Run-time dtypes to typed pointers: f(const uint8_t * | const uint16_t *) and
// f(const float * | const int16_t *, mask as before).  A null mask stays const uint8_t *.
template <typename F>
int with_mask_type(bool has_mask, int mask_dtype, const void *msk, F &&f) {
  if (has_mask && mask_dtype == IFE_U16) return f((const uint16_t *)msk);
  return f((const uint8_t *)msk);
}
template <typename F>
int with_types(int image_dtype, const void *img, bool has_mask, int mask_dtype, const void *msk, F &&f) {
  return with_mask_type(has_mask, mask_dtype, msk, [&](auto m) {
    return image_dtype == IFE_F32 ? f((const float *)img, m) : f((const int16_t *)img, m);
  });
}

// Stage a host input on the device (HOST mode) or pass the device pointer through.
int stage_in(ife_ctx *ctx, int mem, const void *src, size_t bytes, DevBuf &buf, const void **dev) {
  if (src == nullptr) { *dev = nullptr; return IFE_OK; }
  if (mem == IFE_MEM_DEVICE) { *dev = src; return IFE_OK; }
  int rc = ensure(ctx, buf, bytes);
  if (rc) return rc;
  IFE_HIP(ctx, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  *dev = buf.p;
  return IFE_OK;
}

int stage_out_begin(ife_ctx *ctx, int mem, void *dst, size_t bytes, void **dev) {
  if (mem == IFE_MEM_DEVICE) { *dev = dst; return IFE_OK; }
  int rc = ensure(ctx, ctx->st_out, bytes);
  if (rc) return rc;
  *dev = ctx->st_out.p;
  return IFE_OK;
}

int stage_out_end(ife_ctx *ctx, int mem, void *dst, size_t bytes) {
  if (mem == IFE_MEM_DEVICE) return IFE_OK;
  IFE_HIP(ctx, hipMemcpyAsync(dst, ctx->st_out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return IFE_OK;
}

int bind(ife_ctx *ctx) {
  if (!ctx) return IFE_E_ARG;
  IFE_HIP(ctx, hipSetDevice(ctx->device));
  // hipGetLastError() after a launch must report THAT launch: drop whatever an earlier call of
  // this thread (ours or another library's) left pending
  (void)hipGetLastError();
  return IFE_OK;
}

}  // namespace

// =====================================================================================
extern "C" {

int ife_abi_version(void) { return IFE_ABI_VERSION; }

int ife_ctx_create(int device, ife_ctx **out) {
  if (!out) return fail(nullptr, IFE_E_ARG, "ctx out pointer is null");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, IFE_E_HIP, "no HIP device available (%s); this library has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (device < 0 || device >= count)
    return fail(nullptr, IFE_E_ARG, "device %d out of range (0..%d)", device, count - 1);
  hipDeviceProp_t prop;
  IFE_HIP(nullptr, hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, IFE_E_HIP, "device %d is %s; this library is built for gfx950 only",
                device, prop.gcnArchName);
  IFE_HIP(nullptr, hipSetDevice(device));
  ife_ctx *c = new (std::nothrow) ife_ctx();
  if (!c) return fail(nullptr, IFE_E_NOMEM, "host allocation failed");
  c->device = device;
  // IFE_TRIG_MODE in the environment sets the initial IFE_OPT_TRIG_MODE, for callers that
  // cannot reach ife_ctx_set_option (the drop-in tools); set_option still overrides it.
  if (const char *e = getenv("IFE_TRIG_MODE"))
    if ((e[0] == '0' || e[0] == '1' || e[0] == '2') && e[1] == 0) c->trig_mode = e[0] - '0';
  *out = c;
  return IFE_OK;
}

void ife_ctx_destroy(ife_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto e : ctx->sc_done) (void)hipEventDestroy(e);
  if (ctx->sc_copy) (void)hipStreamDestroy(ctx->sc_copy);
  dense_stream_release(ctx);
  if (ctx->ds.copy) (void)hipStreamDestroy(ctx->ds.copy);
  if (ctx->rs_up) (void)hipEventDestroy(ctx->rs_up);
  if (ctx->bs_up) (void)hipEventDestroy(ctx->bs_up);
  for (auto &r : ctx->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
  delete ctx;  // every DevBuf of the context frees itself here, behind the events and streams
}

const char *ife_last_error(const ife_ctx *ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int ife_ctx_set_stream(ife_ctx *ctx, void *hip_stream) {
  if (!ctx) return IFE_E_ARG;
  ctx->stream = (hipStream_t)hip_stream;
  return IFE_OK;
}

int ife_ctx_set_option(ife_ctx *ctx, int option, int value) {
  if (!ctx) return IFE_E_ARG;
  switch (option) {
    case IFE_OPT_TRIG_MODE:
      if (value < 0 || value > 2) return fail(ctx, IFE_E_ARG, "trig mode must be 0, 1 or 2");
      ctx->trig_mode = value;
      return IFE_OK;
    case IFE_OPT_DSCALE_MODE:
      if (value != 0 && value != 1) return fail(ctx, IFE_E_ARG, "dscale mode must be 0 or 1");
      ctx->dscale_mode = value;
      return IFE_OK;
    case IFE_OPT_PROFILE:
      ctx->profile = value ? 1 : 0;
      return IFE_OK;
    case IFE_OPT_ZCHUNK:
      if (value < 1) return fail(ctx, IFE_E_ARG, "zchunk must be >= 1");
      ctx->zchunk = value;
      return IFE_OK;
    case IFE_OPT_IIR_FMA:
      ctx->iir_fma = value ? 1 : 0;
      return IFE_OK;
    case IFE_OPT_IIR_CKPT:
      if (value != 1 && value != 2) return fail(ctx, IFE_E_ARG, "iir checkpoint stride must be 1 or 2");
      ctx->iir_ckpt = value;
      return IFE_OK;
    case IFE_OPT_CONST_LINES:
      ctx->const_lines = value ? 1 : 0;
      return IFE_OK;
    case IFE_OPT_FUSED_DIVIDE:
      ctx->fused_divide = value ? 1 : 0;
      return IFE_OK;
    case IFE_OPT_FEAT_RING:
      ctx->feat_ring = value ? 1 : 0;
      return IFE_OK;
    case IFE_OPT_Z_SWEEP:
      ctx->z_sweep = value ? 1 : 0;
      return IFE_OK;
    case IFE_OPT_DIFFERENTIAL:
      if (value != 0 && value != 1) return fail(ctx, IFE_E_ARG, "the differential option must be 0 or 1");
      ctx->differential = value;
      return IFE_OK;
    case IFE_OPT_DENSE_SCRATCH_MB:
      if (value < 0) return fail(ctx, IFE_E_ARG, "the dense scratch bound must be >= 0 MiB");
      ctx->dense_scratch_mb = value;
      return IFE_OK;
    case IFE_OPT_IIR_BLOCK:
      if (value != 0 && value != 8 && value != 10 && value != 12 && value != 16)
        return fail(ctx, IFE_E_ARG, "iir block must be 0 (per axis), 8, 10, 12 (strided axes only; x keeps 16) or 16");
      ctx->iir_block = value;
      return IFE_OK;
  }
  return fail(ctx, IFE_E_ARG, "unknown option %d", option);
}

int ife_ctx_reserve(ife_ctx *ctx, const ife_volume_desc *vol) {
  int rc = bind(ctx);
  if (rc) return rc;
  rc = check_vol(ctx, vol, false);
  if (rc) return rc;
  return reserve_smooth(ctx, vol);
}

int ife_ctx_synchronize(ife_ctx *ctx) {
  int rc = bind(ctx);
  if (rc) return rc;
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return IFE_OK;
}

// ---- a1 / a2 ------------------------------------------------------------------------
static int eig_batch(ife_ctx *ctx, const float *A6, int64_t n, float *outv, int mem, int nout) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!A6 || !outv))) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mem(ctx, mem))) return rc;
  if (n == 0) return IFE_OK;
  const void *dA;
  void *dO;
  rc = stage_in(ctx, mem, A6, (size_t)n * 6 * 4, ctx->st_img, &dA);
  if (!rc) rc = stage_out_begin(ctx, mem, outv, (size_t)n * nout * 4, &dO);
  if (rc) return rc;
  {
    ProfScope ps(ctx, KK_EIG_BATCH);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (nout == 3)
      hipLaunchKernelGGL((eig_batch_kernel<3>), dim3(blocks), dim3(256), 0, ctx->stream,
                         (const float *)dA, (float *)dO, n, ctx->trig_mode);
    else
      hipLaunchKernelGGL((eig_batch_kernel<6>), dim3(blocks), dim3(256), 0, ctx->stream,
                         (const float *)dA, (float *)dO, n, ctx->trig_mode);
    IFE_HIP(ctx, hipGetLastError());
  }
  return stage_out_end(ctx, mem, outv, (size_t)n * nout * 4);
}

int ife_eigenvalues(ife_ctx *ctx, const float *A6, int64_t n, float *ev3, int mem) {
  return eig_batch(ctx, A6, n, ev3, mem, 3);
}
int ife_eigenvalue_features(ife_ctx *ctx, const float *A6, int64_t n, float *f6, int mem) {
  return eig_batch(ctx, A6, n, f6, mem, 6);
}

// ---- a3 -----------------------------------------------------------------------------
int ife_hessian3d(ife_ctx *ctx, const float *image, const ife_volume_desc *vol, float *out6,
                  int layout, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_layout_mem(ctx, layout, mem))) return rc;
  if (!image || !out6) return fail(ctx, IFE_E_ARG, "null pointer");
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dI;
  void *dO;
  if ((rc = stage_in(ctx, mem, image, n * 4, ctx->st_img, &dI))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out6, n * 24, &dO))) return rc;
  rc = launch_features<FEAT_HESSIAN6>(ctx, ValRaw<float>{(const float *)dI},
                                      (const uint8_t *)nullptr, (float *)dO, vol, layout);
  if (rc) return rc;
  return stage_out_end(ctx, mem, out6, n * 24);
}

int ife_gradient_magnitude(ife_ctx *ctx, const float *image, const ife_volume_desc *vol,
                           float *out, int mem) {
  return ife_fd_gradient_features(ctx, image, nullptr, vol, out, mem);
}

// ---- a4 -----------------------------------------------------------------------------
int ife_normalized_gaussian_convolution(ife_ctx *ctx, const float *image,
                                        const float *certainty, const ife_volume_desc *vol,
                                        double sigma, float *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, true))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!image || !certainty || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_sigma(ctx, sigma))) return rc;
  if ((rc = ife_ctx_reserve(ctx, vol))) return rc;
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dI, *dC;
  void *dO;
  if ((rc = stage_in(ctx, mem, image, n * 4, ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, certainty, n * 4, ctx->st_aux, &dC))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out, n * 4, &dO))) return rc;
  float *tc = (float *)ctx->pre[0].p;
  rc = launch_prep<float, float>(ctx, (const float *)dI, (const float *)dC, tc, nullptr,
                                 (int64_t)n);
  const double sg = sigma;
  if (!rc) rc = smooth_group(ctx, tc, (const float *)dC, vol, &sg, 1);
  if (rc) return rc;
  const float *num = (const float *)ctx->fld[0][0].p, *den = (const float *)ctx->fld[0][2].p;
  if (slots_hold_quotient(ctx, true)) {  // the last axis pass has divided already
    IFE_HIP(ctx, hipMemcpyAsync(dO, num, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    ProfScope ps(ctx, KK_DIVIDE);
    hipLaunchKernelGGL(divide_kernel, dim3(2048), dim3(256), 0, ctx->stream, num, den,
                       (float *)dO, (int64_t)n);
    IFE_HIP(ctx, hipGetLastError());
  }
  return stage_out_end(ctx, mem, out, n * 4);
}

// ---- f4: differential normalized convolution ------------------------------------------
int ife_differential_normalized_convolution(ife_ctx *ctx, const float *image,
                                            const float *certainty, const ife_volume_desc *vol,
                                            double sigma, int axis, float *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, true))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!image || !certainty || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_sigma(ctx, sigma))) return rc;
  if ((rc = check_axis(ctx, axis))) return rc;
  if ((rc = ensure_slots(ctx, vol, 2))) return rc;
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dI, *dC;
  void *dO;
  if ((rc = stage_in(ctx, mem, image, n * 4, ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, certainty, n * 4, ctx->st_aux, &dC))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out, n * 4, &dO))) return rc;
  if ((rc = ensure(ctx, ctx->pre[0], n * sizeof(float)))) return rc;
  float *tc = (float *)ctx->pre[0].p;
  if ((rc = launch_prep<float, float>(ctx, (const float *)dI, (const float *)dC, tc, nullptr, (int64_t)n)))
    return rc;
  // four fields through the three axis passes in one launch each: a*cT, a*c, a_x*cT, a_x*c
  // (slot 0: the 0th-order pair, slot 1: the pair differentiated along `axis`)
  const float *in[4];
  float *o[4];
  const double sg[4] = {sigma, sigma, sigma, sigma};
  const int pass_axis[3] = {2, 0, 1};  // SmoothingRecursiveGaussianImageFilter: z, x, y
  for (int p = 0; p < 3 && !rc; ++p) {
    const int a = pass_axis[p];
    const int ord[4] = {0, 0, a == axis ? 1 : 0, a == axis ? 1 : 0};
    for (int j = 0; j < 4; ++j) {
      const int slot = j / 2, f = j % 2;
      const int src = (p % 2 == 0) ? 1 : 0, dst = (p % 2 == 0) ? 0 : 1;  // ping-pong: ->0, ->1, ->0
      in[j] = p == 0 ? (f == 0 ? tc : (const float *)dC) : (const float *)ctx->fld[slot][2 * f + src].p;
      o[j] = (float *)ctx->fld[slot][2 * f + dst].p;
    }
    rc = launch_iir(ctx, vol, a, 4, in, o, sg, 1, ord);
  }
  if (rc) return rc;
  {
    ProfScope ps(ctx, KK_DIVIDE);
    hipLaunchKernelGGL(diffconv_kernel, dim3(2048), dim3(256), 0, ctx->stream,
                       (const float *)ctx->fld[0][0].p, (const float *)ctx->fld[0][2].p,
                       (const float *)ctx->fld[1][0].p, (const float *)ctx->fld[1][2].p,
                       (float)(1.0 / (axis == 0 ? vol->sx : axis == 1 ? vol->sy : vol->sz)), (float *)dO,
                       (int64_t)n);
    IFE_HIP(ctx, hipGetLastError());
  }
  return stage_out_end(ctx, mem, out, n * 4);
}

// ---- a6 -----------------------------------------------------------------------------
int ife_fd_hessian_features(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                            int mask_dtype, const ife_volume_desc *vol, float *out6, int layout,
                            int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_layout_mem(ctx, layout, mem))) return rc;
  if (!image || !out6) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_image_dtype(ctx, image_dtype))) return rc;
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, true))) return rc;
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dI, *dM;
  void *dO;
  if ((rc = stage_in(ctx, mem, image, n * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, mask, n * (mask ? dtype_size(mask_dtype) : 0), ctx->st_mask, &dM)))
    return rc;
  if ((rc = stage_out_begin(ctx, mem, out6, n * 24, &dO))) return rc;
  rc = with_types(image_dtype, dI, mask != nullptr, mask_dtype, dM, [&](auto img, auto msk) {
    using TI = std::remove_cv_t<std::remove_pointer_t<decltype(img)>>;
    return launch_features<FEAT_EIG6>(ctx, ValRaw<TI>{img}, msk, (float *)dO, vol, layout);
  });
  if (rc) return rc;
  return stage_out_end(ctx, mem, out6, n * 24);
}

// ---- a7 -----------------------------------------------------------------------------
int ife_fd_gradient_features(ife_ctx *ctx, const float *image, const float *mask,
                             const ife_volume_desc *vol, float *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!image || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dI, *dM;
  void *dO;
  if ((rc = stage_in(ctx, mem, image, n * 4, ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, mask, mask ? n * 4 : 0, ctx->st_aux, &dM))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out, n * 4, &dO))) return rc;
  rc = launch_features<FEAT_GRADMAG>(ctx, ValRaw<float>{(const float *)dI}, (const float *)dM,
                                     (float *)dO, vol, IFE_PLANAR);
  if (rc) return rc;
  return stage_out_end(ctx, mem, out, n * 4);
}

// ---- a8 -----------------------------------------------------------------------------
int ife_mask_image_f64(ife_ctx *ctx, const double *image, const double *mask, double outside,
                       int64_t n, double *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!image || !mask || !out))) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mem(ctx, mem))) return rc;
  if (n == 0) return IFE_OK;
  const void *dI, *dM;
  void *dO;
  if ((rc = stage_in(ctx, mem, image, (size_t)n * 8, ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, mask, (size_t)n * 8, ctx->st_aux, &dM))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out, (size_t)n * 8, &dO))) return rc;
  {
    ProfScope ps(ctx, KK_MASK);
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(mask_f64_kernel, dim3(blocks), dim3(256), 0, ctx->stream,
                       (const double *)dI, (const double *)dM, outside, (double *)dO, n);
    IFE_HIP(ctx, hipGetLastError());
  }
  return stage_out_end(ctx, mem, out, (size_t)n * 8);
}

// ---- stage entry points (device pointers only; Z-slab orchestration) --------------------
int ife_stage_prepare(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                      int mask_dtype, const ife_volume_desc *slab, int y_chunks, float *tc,
                      float *cf) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, slab, false))) return rc;
  if (!image || !tc) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_image_dtype(ctx, image_dtype))) return rc;
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, true))) return rc;
  if (y_chunks < 1 || slab->ny % y_chunks)
    return fail(ctx, IFE_E_SIZE, "ny must be a multiple of the number of Y chunks");
  const int64_t n = slab->nx * slab->ny * slab->nz;
  const PrepGeom pg{slab->nx, slab->ny, slab->nz, y_chunks, slab->ny / y_chunks};
  return with_types(image_dtype, image, mask != nullptr, mask_dtype, mask,
                    [&](auto img, auto msk) { return launch_prep(ctx, img, msk, tc, cf, n, pg); });
}

int ife_stage_recursive_gaussian(ife_ctx *ctx, const float *in, float *out,
                                 const ife_volume_desc *vol, int axis, double sigma) {
  return ife_stage_recursive_gaussian_order(ctx, in, out, vol, axis, sigma, 0);
}

int ife_stage_recursive_gaussian_order(ife_ctx *ctx, const float *in, float *out,
                                       const ife_volume_desc *vol, int axis, double sigma, int order) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if (!in || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if (in == out) return fail(ctx, IFE_E_ARG, "the axis pass is not in place");
  if ((rc = check_axis(ctx, axis))) return rc;
  if ((rc = check_sigma(ctx, sigma))) return rc;
  if ((rc = check_axis_len(ctx, vol, axis))) return rc;
  if (order < 0 || order > 2) return fail(ctx, IFE_E_ARG, "the order of the recursive Gaussian must be 0, 1 or 2");
  const float *ins[1] = {in};
  float *outs[1] = {out};
  return launch_iir(ctx, vol, axis, 1, ins, outs, &sigma, 1, &order);
}

int ife_stage_recursive_gaussian_batch(ife_ctx *ctx, int njobs, const float *const *in,
                                       float *const *out, const ife_volume_desc *vol, int axis,
                                       const double *sigmas, int in_y_chunks) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if (!in || !out || !sigmas) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_axis(ctx, axis))) return rc;
  for (int j = 0; j < njobs; ++j)
    if ((rc = check_sigma(ctx, sigmas[j]))) return rc;
  if ((rc = check_axis_len(ctx, vol, axis))) return rc;
  return launch_iir(ctx, vol, axis, njobs, in, out, sigmas, in_y_chunks);
}

size_t ife_stage_z_ck_bytes(const ife_volume_desc *slab) {
  if (!slab || slab->nx <= 0 || slab->ny <= 0 || slab->nz <= 0) return 0;
  return zslab_ck_bytes(slab);
}

int ife_stage_z_sweep_order(ife_ctx *ctx, int direction, int njobs, const float *const *in,
                            const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                            const double *sigmas, const int *orders, int has_neighbour,
                            const void *state_in, void *state_out, void *const *ck) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, slab, false))) return rc;
  if (direction != 0 && direction != 1) return fail(ctx, IFE_E_ARG, "direction must be 0 (causal) or 1 (anticausal)");
  return launch_zslab(ctx, direction, njobs, in, nullptr, slab, line0, nlines, sigmas,
                      direction == 0 ? has_neighbour : 0, direction == 1 ? has_neighbour : 0, state_in,
                      state_out, ck, orders);
}

int ife_stage_z_sweep(ife_ctx *ctx, int direction, int njobs, const float *const *in,
                      const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                      const double *sigmas, int has_neighbour, const void *state_in,
                      void *state_out, void *const *ck) {
  return ife_stage_z_sweep_order(ctx, direction, njobs, in, slab, line0, nlines, sigmas, nullptr, has_neighbour,
                                 state_in, state_out, ck);
}

int ife_stage_z_combine_order(ife_ctx *ctx, int njobs, const float *const *in, float *const *out,
                              const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                              const double *sigmas, const int *orders, int has_lo, int has_hi,
                              void *const *ck) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, slab, false))) return rc;
  return launch_zslab(ctx, 2, njobs, in, out, slab, line0, nlines, sigmas, has_lo, has_hi, nullptr,
                      nullptr, ck, orders);
}

int ife_stage_z_combine(ife_ctx *ctx, int njobs, const float *const *in, float *const *out,
                        const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                        const double *sigmas, int has_lo, int has_hi, void *const *ck) {
  return ife_stage_z_combine_order(ctx, njobs, in, out, slab, line0, nlines, sigmas, nullptr, has_lo, has_hi, ck);
}

int ife_stage_z_fused_order(ife_ctx *ctx, int direction, int njobs, const float *const *in,
                            float *const *out, const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                            const double *sigmas, const int *orders, int has_lo, int has_hi,
                            const void *state_in, void *state_out, void *const *ck) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, slab, false))) return rc;
  if (direction != 0 && direction != 1) return fail(ctx, IFE_E_ARG, "direction must be 0 (causal) or 1 (anticausal)");
  return launch_zslab(ctx, 3 + direction, njobs, in, out, slab, line0, nlines, sigmas, has_lo, has_hi,
                      state_in, state_out, ck, orders);
}

int ife_stage_z_fused(ife_ctx *ctx, int direction, int njobs, const float *const *in,
                      float *const *out, const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                      const double *sigmas, int has_lo, int has_hi, const void *state_in,
                      void *state_out, void *const *ck) {
  return ife_stage_z_fused_order(ctx, direction, njobs, in, out, slab, line0, nlines, sigmas, nullptr, has_lo,
                                 has_hi, state_in, state_out, ck);
}

int ife_stage_recursive_gaussian_quotient(ife_ctx *ctx, int njobs, const float *const *num,
                                          const float *const *den, float *const *out,
                                          const ife_volume_desc *vol, int axis, const double *sigmas) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if (!num || !den || !out || !sigmas) return fail(ctx, IFE_E_ARG, "null pointer");
  if (axis != 1 && axis != 2) return fail(ctx, IFE_E_ARG, "the quotient form runs on the strided axes: 1 (y) or 2 (z)");
  for (int j = 0; j < njobs; ++j)
    if ((rc = check_sigma(ctx, sigmas[j]))) return rc;
  if ((rc = check_axis_len(ctx, vol, axis))) return rc;
  return launch_iir(ctx, vol, axis, njobs, num, out, sigmas, 1, nullptr, den);
}

int ife_stage_features(ife_ctx *ctx, const float *num, const float *den, const void *mask,
                       int mask_dtype, const ife_volume_desc *slab, int halo_lo, int halo_hi,
                       float *out, int layout) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, slab, false))) return rc;
  if ((rc = check_layout_mem(ctx, layout, IFE_MEM_DEVICE))) return rc;
  if (!num || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, true))) return rc;
  return with_mask_type(mask != nullptr, mask_dtype, mask, [&](auto msk) {
    return launch_features<FEAT_FEATURES8>(ctx, ValSmooth{num, den}, msk, out, slab, layout, halo_lo, halo_hi);
  });
}

// ---- measurement ----------------------------------------------------------------------
int ife_get_kernel_times(ife_ctx *ctx, ife_kernel_time *entries, int max_entries) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = drain_profile(ctx))) return rc;
  int k = 0;
  for (int i = 0; i < KK_COUNT && k < max_entries; ++i) {
    if (ctx->acc_n[i] == 0) continue;
    memset(&entries[k], 0, sizeof entries[k]);
    strncpy(entries[k].name, kKindNames[i], sizeof entries[k].name - 1);
    entries[k].launches = ctx->acc_n[i];
    entries[k].total_ms = ctx->acc_ms[i];
    ++k;
  }
  return k;
}

// The box's own streaming rates, measured with this library's access shape (16 B per lane,
// grid-stride, hipEvents on the context's stream): what the roofline fractions in bench.py are
// read against beside the 8 TB/s peak.
__global__ __launch_bounds__(256) void stream_fill_kernel(float4 *__restrict__ dst, int64_t n4, float v) {
  const float4 x = make_float4(v, v, v, v);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    __builtin_nontemporal_store(f32x4{x.x, x.y, x.z, x.w}, reinterpret_cast<f32x4 *>(dst) + i);
}
__global__ __launch_bounds__(256) void stream_copy_kernel(const float4 *__restrict__ src,
                                                          float4 *__restrict__ dst, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(src) + i),
                                reinterpret_cast<f32x4 *>(dst) + i);
}
int ife_measure_stream(ife_ctx *ctx, int mode, void *dst, const void *src, size_t bytes, int reps,
                       double *ms_per_pass) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!dst || !ms_per_pass || (mode == 1 && !src) || (mode != 0 && mode != 1) || reps < 1)
    return fail(ctx, IFE_E_ARG, "bad arguments");
  if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) % 16 || bytes % 16 || bytes == 0)
    return fail(ctx, IFE_E_ARG, "buffers and size must be multiples of 16 bytes");
  const int64_t n4 = (int64_t)(bytes / 16);
  // one piece per thread: the fastest shape on this chip (see launch_prep)
  const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 0x7fffffff);
  auto launch = [&]() {
    if (mode == 0) hipLaunchKernelGGL(stream_fill_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (float4 *)dst, n4, 1.0f);
    else hipLaunchKernelGGL(stream_copy_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const float4 *)src, (float4 *)dst, n4);
  };
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  float ms = 0.f;
  if (e == hipSuccess) {
    launch();  // warm
    (void)hipEventRecord(a, ctx->stream);
    for (int i = 0; i < reps; ++i) launch();
    (void)hipEventRecord(b, ctx->stream);
    e = hipEventSynchronize(b);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  }
  if (a) (void)hipEventDestroy(a);  // whatever was created, on every path
  if (b) (void)hipEventDestroy(b);
  if (e != hipSuccess) return fail(ctx, IFE_E_HIP, "stream measurement: %s", hipGetErrorString(e));
  *ms_per_pass = (double)ms / reps;
  return IFE_OK;
}

int ife_reset_kernel_times(ife_ctx *ctx) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = drain_profile(ctx))) return rc;
  for (int i = 0; i < KK_COUNT; ++i) { ctx->acc_ms[i] = 0; ctx->acc_n[i] = 0; }
  return IFE_OK;
}

}  // extern "C"

#include "diff_capi.inc"    // the jet of one scale
#include "scales_capi.inc"  // the scale loop over both paths, before its users: the sample and dense calls
#include "scale_select_capi.inc"  // a fourth sink of the scale loop
#include "deflate_capi.inc"  // reads the scale stream
#include "stats_capi.inc"
#include "distance_capi.inc"
#include "resample_capi.inc"
#include "bspline_capi.inc"  // shares the resampling checks
#include "dense_capi.inc"
#include "labels_capi.inc"  // shares the dense centres, budget and x / y passes
#include "region_capi.inc"
#include "sampling_capi.inc"  // shares the dense geometry and the scans
#include "coverage_capi.inc"  // shares the sort, the scans and the overlap check
#include "multi_capi.inc"
