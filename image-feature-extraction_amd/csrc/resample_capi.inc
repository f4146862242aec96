// resample_capi.inc -- ife_resample / ife_resample_f64 (include/ife_hip.h): a volume brought onto
// another grid through an axis-aligned translation, linear or nearest; included at the end of
// ife_capi.hip (shares its context and staging helpers).  The launch records no profiling kind.

#include <cfloat>
#include <limits>

namespace {

struct ResampleArgs {
  const ife_volume_desc *src_vol, *dst_vol;
  const double *src_origin, *dst_origin, *translation;
  int interpolation, mem;
  double default_value;
};

bool rs_finite3(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// is `d` a value of T?  (the comparison with the limits comes first: no conversion out of range)
template <typename T>
bool rs_representable(double d) {
  if constexpr (std::is_floating_point<T>::value)
    return std::is_same<T, double>::value || (std::fabs(d) <= (double)FLT_MAX && (double)(float)d == d);
  else
    return d >= (double)std::numeric_limits<T>::min() && d <= (double)std::numeric_limits<T>::max() &&
           d == std::floor(d);
}

// Everything that is refused, before anything is staged or written.  es / eo: element sizes of
// source and output.
int rs_check(ife_ctx *ctx, const void *src, const void *out, const ResampleArgs &a, size_t es, size_t eo) {
  if (!src || !out || !a.src_vol || !a.dst_vol || !a.src_origin || !a.dst_origin || !a.translation)
    return fail(ctx, IFE_E_ARG, "null pointer");
  int rc = check_vol(ctx, a.src_vol, false);
  if (rc) return rc;
  if ((rc = check_vol(ctx, a.dst_vol, false))) return rc;
  if (a.interpolation != IFE_INTERP_LINEAR && a.interpolation != IFE_INTERP_NEAREST)
    return fail(ctx, IFE_E_ARG, "bad interpolation %d", a.interpolation);
  if ((rc = check_mem(ctx, a.mem))) return rc;
  if (!rs_finite3(a.src_origin) || !rs_finite3(a.dst_origin) || !rs_finite3(a.translation) ||
      !std::isfinite(a.default_value))
    return fail(ctx, IFE_E_ARG, "origins, translation and default value must be finite");
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), o0 = reinterpret_cast<uintptr_t>(out);
  if (a.mem == IFE_MEM_DEVICE && (s0 % es || o0 % eo))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  const uintptr_t sb = (uintptr_t)(a.src_vol->nx * a.src_vol->ny * a.src_vol->nz) * es;
  const uintptr_t ob = (uintptr_t)(a.dst_vol->nx * a.dst_vol->ny * a.dst_vol->nz) * eo;
  if (s0 < o0 + ob && o0 < s0 + sb) return fail(ctx, IFE_E_ARG, "source and output overlap");
  return IFE_OK;
}

// The three axis tables, x then y then z, built in the context's host buffer and uploaded behind
// whatever the stream holds.  The host buffer is read by that upload after this returns: the
// next call waits for the event before it writes the buffer again, and the context outlives it.
int rs_tables(ife_ctx *ctx, const ResampleArgs &a, const ResampleEntry **tx, const ResampleEntry **ty,
              const ResampleEntry **tz) {
  const ife_volume_desc &s = *a.src_vol, &t = *a.dst_vol;
  const size_t n = (size_t)(t.nx + t.ny + t.nz);
  if (ctx->rs_up) IFE_HIP(ctx, hipEventSynchronize(ctx->rs_up));
  else IFE_HIP(ctx, hipEventCreateWithFlags(&ctx->rs_up, hipEventDisableTiming));
  try {
    ctx->rs_host.resize(n);
  } catch (const std::bad_alloc &) {
    return fail(ctx, IFE_E_NOMEM, "host allocation failed");
  }
  ResampleEntry *h = ctx->rs_host.data();
  resample_axis_table(t.nx, s.nx, s.sx, a.src_origin[0], t.sx, a.dst_origin[0], a.translation[0], h);
  resample_axis_table(t.ny, s.ny, s.sy, a.src_origin[1], t.sy, a.dst_origin[1], a.translation[1], h + t.nx);
  resample_axis_table(t.nz, s.nz, s.sz, a.src_origin[2], t.sz, a.dst_origin[2], a.translation[2],
                      h + t.nx + t.ny);
  int rc = ensure(ctx, ctx->rs_tab, n * sizeof(ResampleEntry));
  if (rc) return rc;
  IFE_HIP(ctx, hipMemcpyAsync(ctx->rs_tab.p, h, n * sizeof(ResampleEntry), hipMemcpyHostToDevice, ctx->stream));
  IFE_HIP(ctx, hipEventRecord(ctx->rs_up, ctx->stream));
  *tx = (const ResampleEntry *)ctx->rs_tab.p;
  *ty = *tx + t.nx;
  *tz = *ty + t.ny;
  return IFE_OK;
}

template <typename TS, typename TO, int INTERP>
int rs_launch(ife_ctx *ctx, const TS *src, TO *out, const ResampleArgs &a, const ResampleEntry *tx,
              const ResampleEntry *ty, const ResampleEntry *tz) {
  const int64_t rows = a.dst_vol->ny * a.dst_vol->nz;
  const unsigned blocks = (unsigned)std::min<int64_t>(rows, RS_MAX_BLOCKS);
  hipLaunchKernelGGL((resample_kernel<TS, TO, INTERP>), dim3(blocks), dim3(RS_THREADS), 0, ctx->stream, src, out, tx,
                     ty, tz, a.dst_vol->nx, a.dst_vol->ny, rows, a.src_vol->nx, a.src_vol->ny,
                     (TO)a.default_value);
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

// checks, staging, tables and launch for a source type; linear writes TL, nearest the source type
template <typename TS, typename TL>
int rs_run(ife_ctx *ctx, const void *src, void *out, const ResampleArgs &a) {
  const bool linear = a.interpolation == IFE_INTERP_LINEAR;
  const size_t es = sizeof(TS), eo = linear ? sizeof(TL) : sizeof(TS);
  int rc = rs_check(ctx, src, out, a, es, eo);
  if (rc) return rc;
  if (!(linear ? rs_representable<TL>(a.default_value) : rs_representable<TS>(a.default_value)))
    return fail(ctx, IFE_E_ARG, "the default value %g is not a value of the output type", a.default_value);
  const size_t sb = (size_t)(a.src_vol->nx * a.src_vol->ny * a.src_vol->nz) * es;
  const size_t ob = (size_t)(a.dst_vol->nx * a.dst_vol->ny * a.dst_vol->nz) * eo;
  const void *dS;
  void *dO;
  const ResampleEntry *tx, *ty, *tz;
  if ((rc = stage_in(ctx, a.mem, src, sb, ctx->st_img, &dS))) return rc;
  if ((rc = stage_out_begin(ctx, a.mem, out, ob, &dO))) return rc;
  if ((rc = rs_tables(ctx, a, &tx, &ty, &tz))) return rc;
  rc = linear ? rs_launch<TS, TL, 0>(ctx, (const TS *)dS, (TL *)dO, a, tx, ty, tz)
              : rs_launch<TS, TS, 1>(ctx, (const TS *)dS, (TS *)dO, a, tx, ty, tz);
  if (rc) return rc;
  return stage_out_end(ctx, a.mem, out, ob);
}

}  // namespace

extern "C" {

// ---- itk::ResampleImageFilter with a TranslationTransform (tools/Resample.cxx:83-99) ----------
int ife_resample(ife_ctx *ctx, const void *src, int src_dtype, const ife_volume_desc *src_vol,
                 const double src_origin[3], const ife_volume_desc *dst_vol, const double dst_origin[3],
                 const double translation[3], int interpolation, double default_value, void *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  const ResampleArgs a{src_vol, dst_vol, src_origin, dst_origin, translation, interpolation, mem, default_value};
  switch (src_dtype) {
    case IFE_F32: return rs_run<float, float>(ctx, src, out, a);
    case IFE_I16: return rs_run<int16_t, float>(ctx, src, out, a);
    case IFE_U8: return rs_run<uint8_t, float>(ctx, src, out, a);
    case IFE_U16: return rs_run<uint16_t, float>(ctx, src, out, a);
  }
  return fail(ctx, IFE_E_ARG, "source dtype must be IFE_F32, IFE_I16, IFE_U8 or IFE_U16");
}

int ife_resample_f64(ife_ctx *ctx, const double *src, const ife_volume_desc *src_vol, const double src_origin[3],
                     const ife_volume_desc *dst_vol, const double dst_origin[3], const double translation[3],
                     int interpolation, double default_value, double *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  const ResampleArgs a{src_vol, dst_vol, src_origin, dst_origin, translation, interpolation, mem, default_value};
  return rs_run<double, double>(ctx, src, out, a);
}

}  // extern "C"
