// bspline_capi.inc -- ife_bspline_coefficients*, ife_resample_bspline* and ife_window_u8
// (include/ife_hip.h): the recursive B-spline prefilter of orders 0 to 5, the gather onto a target
// grid and the 8-bit intensity window; included after resample_capi.inc (shares its checks and
// ife_capi.hip's staging helpers).  The launches record no profiling kind.

namespace {

struct BsplineArgs {
  const ife_volume_desc *src_vol, *dst_vol;
  const double *src_origin, *dst_origin, *translation;
  int order, extrapolate, mem;
  double default_value;
};

int64_t bs_voxels(const ife_volume_desc *v) { return v->nx * v->ny * v->nz; }

unsigned bs_blocks(int64_t items, int64_t per_block, int64_t cap) {
  return (unsigned)std::min<int64_t>((items + per_block - 1) / per_block, cap);
}

int bs_check_order(ife_ctx *ctx, int order) {
  if (order < 0 || order > BS_MAX_ORDER) return fail(ctx, IFE_E_ARG, "spline order %d is outside 0..5", order);
  return IFE_OK;
}

// the prefilter, in place on the doubles at c: x, then y, then z
int bs_prefilter(ife_ctx *ctx, double *c, const ife_volume_desc &v, int order) {
  const int64_t plane = v.nx * v.ny;
  const BsAxis ax = bspline_axis(order, v.nx), ay = bspline_axis(order, v.ny), az = bspline_axis(order, v.nz);
  if (ax.npoles) {
    const int64_t rows = v.ny * v.nz;
    hipLaunchKernelGGL(bspline_x_kernel, dim3(bs_blocks(rows, BSX_ROWS, BS_MAX_LINE_BLOCKS)), dim3(BS_THREADS), 0,
                       ctx->stream, c, ax, v.nx, rows);
    IFE_HIP(ctx, hipGetLastError());
  }
  if (ay.npoles) {
    const int64_t lines = v.nx * v.nz;
    hipLaunchKernelGGL(bspline_strided_kernel, dim3(bs_blocks(lines, BS_THREADS, BS_MAX_LINE_BLOCKS)),
                       dim3(BS_THREADS), 0, ctx->stream, c, ay, v.ny, v.nx, v.nx, plane, lines);
    IFE_HIP(ctx, hipGetLastError());
  }
  if (az.npoles) {
    hipLaunchKernelGGL(bspline_strided_kernel, dim3(bs_blocks(plane, BS_THREADS, BS_MAX_LINE_BLOCKS)),
                       dim3(BS_THREADS), 0, ctx->stream, c, az, v.nz, plane, plane, plane, plane);
    IFE_HIP(ctx, hipGetLastError());
  }
  return IFE_OK;
}

// coefficients of the device source dS into the device doubles dC (dC == dS: in place, doubles)
template <typename TS>
int bs_coefficients_dev(ife_ctx *ctx, const TS *dS, double *dC, const ife_volume_desc &v, int order) {
  const int64_t n = bs_voxels(&v);
  if ((const void *)dS != (const void *)dC) {
    hipLaunchKernelGGL((bspline_convert_kernel<TS>), dim3(bs_blocks(n, BS_THREADS, BS_MAX_LINE_BLOCKS)),
                       dim3(BS_THREADS), 0, ctx->stream, dS, dC, n);
    IFE_HIP(ctx, hipGetLastError());
  }
  return bs_prefilter(ctx, dC, v, order);
}

template <typename TS>
int bs_coefficients_run(ife_ctx *ctx, const void *src, const ife_volume_desc *vol, int order, double *coef, int mem) {
  if (!src || !coef) return fail(ctx, IFE_E_ARG, "null pointer");
  int rc = check_vol(ctx, vol, false);
  if (rc) return rc;
  if ((rc = bs_check_order(ctx, order))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), o0 = reinterpret_cast<uintptr_t>(coef);
  if (mem == IFE_MEM_DEVICE && (s0 % sizeof(TS) || o0 % sizeof(double)))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  const size_t n = (size_t)bs_voxels(vol), sb = n * sizeof(TS), ob = n * sizeof(double);
  const bool in_place = std::is_same<TS, double>::value && s0 == o0;
  if (!in_place && s0 < o0 + ob && o0 < s0 + sb) return fail(ctx, IFE_E_ARG, "source and coefficients overlap");
  const void *dS;
  void *dC;
  if ((rc = stage_in(ctx, mem, src, sb, ctx->st_img, &dS))) return rc;
  if ((rc = stage_out_begin(ctx, mem, coef, ob, &dC))) return rc;
  if ((rc = bs_coefficients_dev<TS>(ctx, (const TS *)dS, (double *)dC, *vol, order))) return rc;
  return stage_out_end(ctx, mem, coef, ob);
}

// Everything ife_resample refuses, with order and extrapolate in the interpolation's place.
int bs_check(ife_ctx *ctx, const void *src, const void *out, const BsplineArgs &a, size_t es, size_t eo) {
  if (!src || !out || !a.src_vol || !a.dst_vol || !a.src_origin || !a.dst_origin || !a.translation)
    return fail(ctx, IFE_E_ARG, "null pointer");
  int rc = check_vol(ctx, a.src_vol, false);
  if (rc) return rc;
  if ((rc = check_vol(ctx, a.dst_vol, false))) return rc;
  if ((rc = bs_check_order(ctx, a.order))) return rc;
  if (a.extrapolate != 0 && a.extrapolate != 1) return fail(ctx, IFE_E_ARG, "bad extrapolate %d", a.extrapolate);
  if ((rc = check_mem(ctx, a.mem))) return rc;
  if (!rs_finite3(a.src_origin) || !rs_finite3(a.dst_origin) || !rs_finite3(a.translation) ||
      !std::isfinite(a.default_value))
    return fail(ctx, IFE_E_ARG, "origins, translation and default value must be finite");
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), o0 = reinterpret_cast<uintptr_t>(out);
  if (a.mem == IFE_MEM_DEVICE && (s0 % es || o0 % eo))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  const uintptr_t sb = (uintptr_t)bs_voxels(a.src_vol) * es, ob = (uintptr_t)bs_voxels(a.dst_vol) * eo;
  if (s0 < o0 + ob && o0 < s0 + sb) return fail(ctx, IFE_E_ARG, "source and output overlap");
  return IFE_OK;
}

// The gather's tables (bspline_plan.hpp) built in the context's host buffer and uploaded behind
// whatever the stream holds: all weights, x then y then z, then all indices, then the edge words.
// The next call waits for the upload's event before it writes the host buffer again.
int bs_tables(ife_ctx *ctx, const BsplineArgs &a, const double **W, const int32_t **I, const int32_t **E) {
  const ife_volume_desc &s = *a.src_vol, &t = *a.dst_vol;
  const size_t K = (size_t)a.order + 1, T = (size_t)(t.nx + t.ny + t.nz);
  const size_t bytes = T * K * sizeof(double) + T * K * sizeof(int32_t) + T * sizeof(int32_t);
  if (ctx->bs_up) IFE_HIP(ctx, hipEventSynchronize(ctx->bs_up));
  else IFE_HIP(ctx, hipEventCreateWithFlags(&ctx->bs_up, hipEventDisableTiming));
  try {
    ctx->bs_host.resize((bytes + sizeof(double) - 1) / sizeof(double));
  } catch (const std::bad_alloc &) {
    return fail(ctx, IFE_E_NOMEM, "host allocation failed");
  }
  double *w = ctx->bs_host.data();
  int32_t *idx = reinterpret_cast<int32_t *>(w + T * K), *edge = idx + T * K;
  const int64_t n_t[3] = {t.nx, t.ny, t.nz}, n_s[3] = {s.nx, s.ny, s.nz};
  const double s_s[3] = {s.sx, s.sy, s.sz}, s_t[3] = {t.sx, t.sy, t.sz};
  size_t at = 0;
  for (int d = 0; d < 3; ++d) {
    bspline_axis_table(a.order, n_t[d], n_s[d], s_s[d], a.src_origin[d], s_t[d], a.dst_origin[d], a.translation[d],
                       w + at * K, idx + at * K, edge + at);
    at += (size_t)n_t[d];
  }
  int rc = ensure(ctx, ctx->bs_tab, bytes);
  if (rc) return rc;
  IFE_HIP(ctx, hipMemcpyAsync(ctx->bs_tab.p, w, bytes, hipMemcpyHostToDevice, ctx->stream));
  IFE_HIP(ctx, hipEventRecord(ctx->bs_up, ctx->stream));
  *W = (const double *)ctx->bs_tab.p;
  *I = reinterpret_cast<const int32_t *>(*W + T * K);
  *E = *I + T * K;
  return IFE_OK;
}

template <typename TS, typename TO, int ORDER>
int bs_gather(ife_ctx *ctx, const double *coef, const TS *src, TO *out, const BsplineArgs &a, const double *W,
              const int32_t *I, const int32_t *E) {
  const ife_volume_desc &s = *a.src_vol, &t = *a.dst_vol;
  const int64_t groups = t.ny * ((t.nz + BS_ZB - 1) / BS_ZB);
  hipLaunchKernelGGL((bspline_gather_kernel<TS, TO, ORDER>), dim3(bs_blocks(groups, 1, BS_MAX_GATHER_BLOCKS)),
                     dim3(BS_THREADS), 0, ctx->stream, coef, src, out, W, I, E, t.nx, t.ny, t.nz, groups, s.nx, s.ny,
                     bspline_taps(ORDER, s.nx), bspline_taps(ORDER, s.ny), bspline_taps(ORDER, s.nz), a.extrapolate,
                     (TO)a.default_value);
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

template <typename TS, typename TO>
int bs_resample_run(ife_ctx *ctx, const void *src, void *out, const BsplineArgs &a) {
  int rc = bs_check(ctx, src, out, a, sizeof(TS), sizeof(TO));
  if (rc) return rc;
  if (!rs_representable<TO>(a.default_value))
    return fail(ctx, IFE_E_ARG, "the default value %g is not a value of the output type", a.default_value);
  const size_t n = (size_t)bs_voxels(a.src_vol), sb = n * sizeof(TS);
  const size_t ob = (size_t)bs_voxels(a.dst_vol) * sizeof(TO);
  const void *dS;
  void *dO;
  const double *W;
  const int32_t *I, *E;
  if ((rc = stage_in(ctx, a.mem, src, sb, ctx->st_img, &dS))) return rc;
  if ((rc = stage_out_begin(ctx, a.mem, out, ob, &dO))) return rc;
  if ((rc = ensure(ctx, ctx->bs_coef, n * sizeof(double)))) return rc;
  double *coef = (double *)ctx->bs_coef.p;
  if ((rc = bs_coefficients_dev<TS>(ctx, (const TS *)dS, coef, *a.src_vol, a.order))) return rc;
  if ((rc = bs_tables(ctx, a, &W, &I, &E))) return rc;
  const TS *s = (const TS *)dS;
  TO *o = (TO *)dO;
  switch (a.order) {
    case 0: rc = bs_gather<TS, TO, 0>(ctx, coef, s, o, a, W, I, E); break;
    case 1: rc = bs_gather<TS, TO, 1>(ctx, coef, s, o, a, W, I, E); break;
    case 2: rc = bs_gather<TS, TO, 2>(ctx, coef, s, o, a, W, I, E); break;
    case 3: rc = bs_gather<TS, TO, 3>(ctx, coef, s, o, a, W, I, E); break;
    case 4: rc = bs_gather<TS, TO, 4>(ctx, coef, s, o, a, W, I, E); break;
    default: rc = bs_gather<TS, TO, 5>(ctx, coef, s, o, a, W, I, E); break;
  }
  if (rc) return rc;
  return stage_out_end(ctx, a.mem, out, ob);
}

}  // namespace

extern "C" {

// ---- itk::BSplineDecompositionImageFilter ------------------------------------------------------
int ife_bspline_coefficients(ife_ctx *ctx, const void *src, int src_dtype, const ife_volume_desc *vol, int order,
                             double *coef, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  switch (src_dtype) {
    case IFE_F32: return bs_coefficients_run<float>(ctx, src, vol, order, coef, mem);
    case IFE_I16: return bs_coefficients_run<int16_t>(ctx, src, vol, order, coef, mem);
    case IFE_U8: return bs_coefficients_run<uint8_t>(ctx, src, vol, order, coef, mem);
    case IFE_U16: return bs_coefficients_run<uint16_t>(ctx, src, vol, order, coef, mem);
  }
  return fail(ctx, IFE_E_ARG, "source dtype must be IFE_F32, IFE_I16, IFE_U8 or IFE_U16");
}

int ife_bspline_coefficients_f64(ife_ctx *ctx, const double *src, const ife_volume_desc *vol, int order,
                                 double *coef, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  return bs_coefficients_run<double>(ctx, src, vol, order, coef, mem);
}

// ---- itk::ResampleImageFilter with a BSplineInterpolateImageFunction (tools/ExtractWindow.cxx) ---
int ife_resample_bspline(ife_ctx *ctx, const void *src, int src_dtype, const ife_volume_desc *src_vol,
                         const double src_origin[3], const ife_volume_desc *dst_vol, const double dst_origin[3],
                         const double translation[3], int order, int extrapolate, double default_value, float *out,
                         int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  const BsplineArgs a{src_vol, dst_vol, src_origin, dst_origin, translation, order, extrapolate, mem, default_value};
  switch (src_dtype) {
    case IFE_F32: return bs_resample_run<float, float>(ctx, src, out, a);
    case IFE_I16: return bs_resample_run<int16_t, float>(ctx, src, out, a);
    case IFE_U8: return bs_resample_run<uint8_t, float>(ctx, src, out, a);
    case IFE_U16: return bs_resample_run<uint16_t, float>(ctx, src, out, a);
  }
  return fail(ctx, IFE_E_ARG, "source dtype must be IFE_F32, IFE_I16, IFE_U8 or IFE_U16");
}

int ife_resample_bspline_f64(ife_ctx *ctx, const double *src, const ife_volume_desc *src_vol,
                             const double src_origin[3], const ife_volume_desc *dst_vol, const double dst_origin[3],
                             const double translation[3], int order, int extrapolate, double default_value,
                             double *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  const BsplineArgs a{src_vol, dst_vol, src_origin, dst_origin, translation, order, extrapolate, mem, default_value};
  return bs_resample_run<double, double>(ctx, src, out, a);
}

// ---- itk::IntensityWindowingImageFilter to unsigned char, then the mask --------------------------
int ife_window_u8(ife_ctx *ctx, const double *src, const double *mask, int64_t n, double window_min,
                  double window_max, uint8_t out_min, uint8_t out_max, uint8_t *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!src || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if (n <= 0) return fail(ctx, IFE_E_SIZE, "the number of values must be positive");
  if (!std::isfinite(window_min) || !std::isfinite(window_max) || !(window_max > window_min))
    return fail(ctx, IFE_E_ARG, "the window must be finite and window_max > window_min");
  if ((rc = check_mem(ctx, mem))) return rc;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), m0 = reinterpret_cast<uintptr_t>(mask),
                  o0 = reinterpret_cast<uintptr_t>(out);
  if (mem == IFE_MEM_DEVICE && (s0 % sizeof(double) || m0 % sizeof(double)))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  const size_t ib = (size_t)n * sizeof(double), ob = (size_t)n;
  if ((s0 < o0 + ob && o0 < s0 + ib) || (mask && m0 < o0 + ob && o0 < m0 + ib))
    return fail(ctx, IFE_E_ARG, "an input and the output overlap");
  const double scale = ((double)out_max - (double)out_min) / (window_max - window_min);
  const double shift = (double)out_min - window_min * scale;
  const void *dS, *dM;
  void *dO;
  if ((rc = stage_in(ctx, mem, src, ib, ctx->st_img, &dS))) return rc;
  if ((rc = stage_in(ctx, mem, mask, ib, ctx->st_mask, &dM))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out, ob, &dO))) return rc;
  hipLaunchKernelGGL(bspline_window_kernel, dim3(bs_blocks(n, BS_THREADS, BS_MAX_LINE_BLOCKS)), dim3(BS_THREADS), 0,
                     ctx->stream, (const double *)dS, (const double *)dM, (uint8_t *)dO, n, window_min, window_max,
                     scale, shift, out_min, out_max);
  IFE_HIP(ctx, hipGetLastError());
  return stage_out_end(ctx, mem, out, ob);
}

}  // extern "C"
