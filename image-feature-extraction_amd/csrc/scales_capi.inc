// scales_capi.inc -- the scale loop: which path produces a scale and what is made of it (DESIGN.md
// section 4 "The scale loop and its sinks"), and the feature volume calls of include/ife_hip.h
// (ife_emphysema_features with its streaming form, ife_differential_features).  Included at the end
// of ife_capi.hip behind diff_capi.inc, in front of stats_capi.inc and dense_capi.inc, whose
// composite calls hand their sinks to feature_scales.
//
// A sink is a small struct with one launch per path and scale: from_smooth(ctx, vol, scale, the
// smoothed field) on the finite-difference path, from_jet(ctx, vol, scale, the twenty fields) on
// the differential one, and jet_ready(ctx), which may refuse before the differential path does
// any work.

namespace {

// A feature volume [scale][8 components] of the caller's layout.
template <typename TM>
struct VolumeSink {
  const TM *mask;
  float *out;
  int layout;
  size_t stride;  // floats per scale
  float *at(int s) const { return out + (size_t)s * stride; }
  int jet_ready(ife_ctx *ctx) const { return check_out_alignment(ctx, out, IFE_NUM_FEATURES, layout); }
  int from_smooth(ife_ctx *ctx, const ife_volume_desc *vol, int s, const ValSmooth &vs) const {
    return launch_features<FEAT_FEATURES8>(ctx, vs, mask, at(s), vol, layout);
  }
  int from_jet(ife_ctx *ctx, const ife_volume_desc *vol, int s, const JetFields &f) const {
    return launch_jet<JET_FEATURES8>(ctx, f, mask, at(s), vol, layout);
  }
};

// Row f1: instead of a feature volume per scale, the features of the sampled voxels go straight
// into eight sample columns per scale (stats_capi.inc).
struct ColumnSink {
  const uint8_t *code;       // per voxel: bit 0 = sample here, bit 1 = label non-zero
  const uint32_t *seg_base;  // exclusive scan of the per-row-segment sample counts
  float *columns;            // column (scale*8 + k) at columns + (scale*8 + k) * stride
  int64_t stride, offset;    // elements between columns, samples already in them
  int gx;                    // row segments of 64 voxels per row
  int64_t nseg;
  float *at(int s) const { return columns + (size_t)s * IFE_NUM_FEATURES * stride; }
  int jet_ready(ife_ctx *) const { return IFE_OK; }
  int from_smooth(ife_ctx *ctx, const ife_volume_desc *vol, int s, const ValSmooth &vs) const {
    return launch_features<FEAT_SAMPLES8>(ctx, vs, code, at(s), vol, IFE_PLANAR, 0, 0, seg_base, stride, offset);
  }
  int from_jet(ife_ctx *ctx, const ife_volume_desc *vol, int s, const JetFields &f) const {
    const JetSampleSink sk = {code, seg_base, at(s), stride, offset, (int)vol->nx, gx, nseg};
    return launch_jet_samples(ctx, f, vol, sk);
  }
};

// The dense bag under IFE_OPT_DIFFERENTIAL (dense_capi.inc): the eight planes of bin codes of a
// scale straight from the twenty fields to code_of(scale) ([8][nvox] bytes), then
// each_scale(scale, those planes, the clamped labels).  edges: [n_sigmas * 8][n_edges], device.
// The finite-difference dense path goes through a feature volume instead.
template <typename C, typename F>
struct CodeSink {
  const uint8_t *clamp;
  const float *edges;
  int n_edges;
  C code_of;
  F each_scale;
  int jet_ready(ife_ctx *) const { return IFE_OK; }
  int from_smooth(ife_ctx *ctx, const ife_volume_desc *, int, const ValSmooth &) const {
    return fail(ctx, IFE_E_STATE, "the bin codes of a scale are formed from the jet only");
  }
  int from_jet(ife_ctx *ctx, const ife_volume_desc *vol, int s, const JetFields &f) {
    const JetCodeSink ck = {edges + (size_t)s * IFE_NUM_FEATURES * n_edges, n_edges, code_of(s),
                            vol->nx * vol->ny * vol->nz};
    int r = launch_jet_codes(ctx, f, clamp, vol, ck);
    if (!r) r = each_scale(s, (const uint8_t *)ck.code, clamp);
    return r;
  }
};

// Everything the scale loop allocates for this volume on the given path, now: a caller that sizes
// a budget from the free device memory does so behind it.
int reserve_scales(ife_ctx *ctx, const ife_volume_desc *vol, bool differential) {
  if (!differential) return reserve_smooth(ctx, vol);
  const size_t pitch = ((size_t)(vol->nx * vol->ny * vol->nz) + 3) / 4 * 4;
  int rc = ensure(ctx, ctx->pre[0], pitch * sizeof(float));
  if (!rc) rc = ensure(ctx, ctx->pre[1], pitch * sizeof(float));
  if (!rc) rc = ensure(ctx, ctx->dj_ws, (size_t)JET_SLOTS * pitch * sizeof(float));
  if (!rc) rc = ensure_ck(ctx, vol, IIR_MAX_JOBS);
  return rc;
}

// Every scale of image and mask (device) into the sink, by finite differences of the smoothed
// field or (`differential`) from the jet of the normalized convolution.  The workspace of the
// finite-difference path is reserved by the caller (reserve_scales).  Behind each scale's sink an
// event is recorded into *scale_done when that is given (the scale stream).
template <typename TI, typename TM, typename Sink>
int feature_scales(ife_ctx *ctx, const TI *img, const TM *msk, const ife_volume_desc *vol, const float *sigmas,
                   int n_sigmas, bool differential, Sink &&sink, std::vector<hipEvent_t> *scale_done) {
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  auto scale_finished = [&]() -> int {
    if (!scale_done) return IFE_OK;
    hipEvent_t e;
    IFE_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    scale_done->push_back(e);
    IFE_HIP(ctx, hipEventRecord(e, ctx->stream));
    return IFE_OK;
  };
  int rc;
  if (differential) {
    if ((rc = check_in_alignment(ctx, img, sizeof(TI), msk, sizeof(TM)))) return rc;
    if ((rc = sink.jet_ready(ctx))) return rc;
    // the sources once, then one scale after the other over the same workspace
    rc = jet_sources(ctx, img, msk, (int64_t)n);
    for (int s = 0; s < n_sigmas && !rc; ++s) {
      JetFields f;
      rc = jet_fields(ctx, (const float *)ctx->pre[0].p, (const float *)ctx->pre[1].p, vol, (double)sigmas[s], &f);
      if (!rc) rc = sink.from_jet(ctx, vol, s, f);
      if (!rc) rc = scale_finished();
    }
    return rc;
  }
  float *tc = (float *)ctx->pre[0].p, *cf = (float *)ctx->pre[1].p;
  // Cast + Multiply once for all scales (the reference redoes them per scale, a9).
  // mask == NULL: certainty == 1 everywhere, image*1 is the image and G(1) is exactly
  // 1.0f at every voxel (DESIGN.md "all-ones certainty"), so the denominator is skipped.
  // IFE_OPT_Z_SWEEP: no prepass -- the first launch of the Z pass reads image and mask itself,
  // leaves the same two sources and carries the causal recursions of all scales of a group
  const bool sweep = ctx->z_sweep && ctx->iir_ckpt == 2;
  ZSweepSrc zs;
  zs.img = img; zs.msk = msk;
  zs.img_dtype = std::is_same<TI, float>::value ? IFE_F32 : IFE_I16;
  zs.msk_dtype = std::is_same<TM, uint16_t>::value ? IFE_U16 : IFE_U8;
  zs.tc = tc; zs.cf = cf;
  zs.nf = msk ? 2 : 1;
  const float *src_num;
  if (msk == nullptr && std::is_same<TI, float>::value) {
    src_num = reinterpret_cast<const float *>(img);
    zs.write_src = false;  // the backward sweeps read the image
  } else {
    if (!sweep && (rc = launch_prep<TI, TM>(ctx, img, msk, tc, msk ? cf : nullptr, (int64_t)n))) return rc;
    src_num = tc;
    zs.write_src = true;  // by the first group of scales
  }
  const bool q = slots_hold_quotient(ctx, msk != nullptr);
  for (int s0 = 0; s0 < n_sigmas; s0 += IFE_MAX_SLOTS) {
    const int ns = std::min(IFE_MAX_SLOTS, n_sigmas - s0);
    double sg[IFE_MAX_SLOTS];
    for (int k = 0; k < ns; ++k) sg[k] = (double)sigmas[s0 + k];
    rc = smooth_group(ctx, src_num, msk ? cf : nullptr, vol, sg, ns, sweep ? &zs : nullptr);
    zs.write_src = false;
    for (int k = 0; k < ns && !rc; ++k) {
      const ValSmooth vs{(const float *)ctx->fld[k][0].p, msk && !q ? (const float *)ctx->fld[k][2].p : nullptr};
      rc = sink.from_smooth(ctx, vol, s0 + k, vs);
      if (!rc) rc = scale_finished();
    }
    if (rc) return rc;
  }
  return IFE_OK;
}

// Every scale of a feature volume from device inputs into dout (device): what the feature volume
// calls do behind their argument checks and their staging, and what a composite call that needs a
// feature volume comes to.
int feature_volumes(ife_ctx *ctx, const void *dI, int image_dtype, const void *dM, int mask_dtype,
                    const ife_volume_desc *vol, const float *sigmas, int n_sigmas, float *dout, int layout,
                    bool differential, std::vector<hipEvent_t> *scale_done = nullptr) {
  int rc = reserve_scales(ctx, vol, differential);
  if (rc) return rc;
  const size_t scale_floats = (size_t)(vol->nx * vol->ny * vol->nz) * IFE_NUM_FEATURES;
  return with_types(image_dtype, dI, dM != nullptr, mask_dtype, dM, [&](auto img, auto msk) {
    using TM = std::remove_cv_t<std::remove_pointer_t<decltype(msk)>>;
    return feature_scales(ctx, img, msk, vol, sigmas, n_sigmas, differential,
                          VolumeSink<TM>{msk, dout, layout, scale_floats}, scale_done);
  });
}

// The arguments of the feature volume calls and of the streaming form (which has no output yet).
int features_check(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                   const ife_volume_desc *vol, const float *sigmas, int n_sigmas, bool have_out, int layout,
                   int mem) {
  int rc;
  if ((rc = check_vol(ctx, vol, true))) return rc;
  if ((rc = check_layout_mem(ctx, layout, mem))) return rc;
  if (!image || !have_out || !sigmas) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_sigmas(ctx, sigmas, n_sigmas))) return rc;
  if ((rc = check_image_dtype(ctx, image_dtype))) return rc;
  return check_mask_dtype(ctx, mask, mask_dtype, true);
}

// ife_emphysema_features and ife_differential_features: check, stage, every scale, copy out.
int features_call(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                  const ife_volume_desc *vol, const float *sigmas, int n_sigmas, float *out, int layout, int mem,
                  bool differential) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = features_check(ctx, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, out != nullptr, layout,
                           mem)))
    return rc;
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  const size_t out_bytes = n * IFE_NUM_FEATURES * 4 * (size_t)n_sigmas;
  const void *dI, *dM;
  void *dO;
  if ((rc = stage_in(ctx, mem, image, n * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, mask, n * (mask ? dtype_size(mask_dtype) : 0), ctx->st_mask, &dM))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out, out_bytes, &dO))) return rc;
  if ((rc = feature_volumes(ctx, dI, image_dtype, dM, mask_dtype, vol, sigmas, n_sigmas, (float *)dO, layout,
                            differential)))
    return rc;
  return stage_out_end(ctx, mem, out, out_bytes);
}

}  // namespace

extern "C" {

// ---- a5 + a9 ------------------------------------------------------------------------
int ife_emphysema_features(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                           int mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                           int n_sigmas, float *out, int layout, int mem) {
  return features_call(ctx, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, out, layout, mem, false);
}

int ife_differential_features(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                              const ife_volume_desc *vol, const float *sigmas, int n_sigmas, float *out,
                              int layout, int mem) {
  return features_call(ctx, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, out, layout, mem, true);
}

// ---- a9, streaming form -------------------------------------------------------------
int ife_emphysema_features_end(ife_ctx *ctx) {
  int rc = bind(ctx);
  if (rc) return rc;
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->sc_copy) IFE_HIP(ctx, hipStreamSynchronize(ctx->sc_copy));
  for (auto e : ctx->sc_done) (void)hipEventDestroy(e);
  ctx->sc_done.clear();
  IFE_HIP(ctx, ctx->sc_out.reset());
  IFE_HIP(ctx, ctx->df_out.reset());  // the blocks of the deflated fetch (deflate_capi.inc)
  ctx->sc_scale_bytes = 0;
  return IFE_OK;
}

int ife_emphysema_features_begin(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                                 int mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                                 int n_sigmas, int layout) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = features_check(ctx, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, true, layout,
                           IFE_MEM_HOST)))
    return rc;
  if ((rc = ife_emphysema_features_end(ctx))) return rc;  // drop an earlier, unfinished run
  // the option as it stands now decides for the whole stream: _fetch only copies what is enqueued here
  const bool differential = ctx->differential != 0;
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  ctx->sc_scale_bytes = n * IFE_NUM_FEATURES * sizeof(float);
  ctx->sc_layout = layout;
  if ((rc = ensure(ctx, ctx->sc_out, ctx->sc_scale_bytes * (size_t)n_sigmas))) return rc;
  if (!ctx->sc_copy) IFE_HIP(ctx, hipStreamCreateWithFlags(&ctx->sc_copy, hipStreamNonBlocking));
  // The caller may reuse image and mask once _begin returns, so it waits for the uploads (not for
  // the scales) before returning: an event behind them, since from page-locked memory the uploads
  // run asynchronously to the host.
  const void *dI, *dM;
  if ((rc = stage_in(ctx, IFE_MEM_HOST, image, n * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, IFE_MEM_HOST, mask, n * (mask ? dtype_size(mask_dtype) : 0), ctx->st_mask, &dM))) {
    (void)hipStreamSynchronize(ctx->stream);  // the image upload may still read the caller's memory
    return rc;
  }
  hipEvent_t uploaded = nullptr;
  if (hipEventCreateWithFlags(&uploaded, hipEventDisableTiming) != hipSuccess ||
      hipEventRecord(uploaded, ctx->stream) != hipSuccess) {
    if (uploaded) (void)hipEventDestroy(uploaded);
    (void)hipStreamSynchronize(ctx->stream);
    return fail(ctx, IFE_E_HIP, "upload event: %s", hipGetErrorString(hipGetLastError()));
  }
  rc = feature_volumes(ctx, dI, image_dtype, dM, mask_dtype, vol, sigmas, n_sigmas, (float *)ctx->sc_out.p, layout,
                       differential, &ctx->sc_done);
  const hipError_t up = hipEventSynchronize(uploaded);
  (void)hipEventDestroy(uploaded);
  if (!rc && up != hipSuccess) rc = fail(ctx, IFE_E_HIP, "upload: %s", hipGetErrorString(up));
  if (rc) (void)ife_emphysema_features_end(ctx);
  return rc;
}

int ife_emphysema_features_fetch(ife_ctx *ctx, int scale, float *out) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!out) return fail(ctx, IFE_E_ARG, "null pointer");
  if (scale < 0 || scale >= (int)ctx->sc_done.size())
    return fail(ctx, IFE_E_STATE, "scale %d was not started by ife_emphysema_features_begin (%d scales)",
                scale, (int)ctx->sc_done.size());
  IFE_HIP(ctx, hipStreamWaitEvent(ctx->sc_copy, ctx->sc_done[scale], 0));
  IFE_HIP(ctx, hipMemcpyAsync(out, (const char *)ctx->sc_out.p + (size_t)scale * ctx->sc_scale_bytes,
                              ctx->sc_scale_bytes, hipMemcpyDeviceToHost, ctx->sc_copy));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->sc_copy));
  return IFE_OK;
}

}  // extern "C"
