// scale_select_capi.inc -- ife_scale_select of include/ife_hip.h (DESIGN.md section 4 "Scale
// selection"); included at the end of ife_capi.hip behind scales_capi.inc, whose scale loop it hands
// a fourth sink.  The checks that need no device are scale_select_plan.hpp's, plain host code.

namespace {

// One scale of features into the one-scale planar workspace by the feature kernels as they are,
// then the fold of that scale into the running maxima.  The eigenvalues are those of the feature
// calls bit for bit because the launches are the feature calls' own.
template <typename TM>
struct SelectSink {
  const TM *mask;
  float *ws;  // [8][nvox], planar
  const float *sigmas;
  const ife_scale_measure *measures;
  int n_measures;
  float *response;  // [n_measures][nvox]
  uint8_t *index;   // the same, or null
  int jet_ready(ife_ctx *) const { return IFE_OK; }
  int from_smooth(ife_ctx *ctx, const ife_volume_desc *vol, int s, const ValSmooth &vs) const {
    int rc = launch_features<FEAT_FEATURES8>(ctx, vs, mask, ws, vol, IFE_PLANAR);
    return rc ? rc : fold(ctx, vol, s);
  }
  int from_jet(ife_ctx *ctx, const ife_volume_desc *vol, int s, const JetFields &f) const {
    int rc = launch_jet<JET_FEATURES8>(ctx, f, mask, ws, vol, IFE_PLANAR);
    return rc ? rc : fold(ctx, vol, s);
  }
  int fold(ife_ctx *ctx, const ife_volume_desc *vol, int s) const {
    const int64_t nvox = vol->nx * vol->ny * vol->nz;
    const int64_t blocks = ((nvox + 3) / 4 + 255) / 256;  // one group of four voxels per lane, no cap
    if (blocks > 0x7fffffff) return fail(ctx, IFE_E_SIZE, "volume too large for the fold kernel grid");
    const SelectPlanes p = {ws + 2 * nvox, ws + 3 * nvox, ws + 4 * nvox, ws + 5 * nvox};
    // lane k starts at element 4k of every array: 16 bytes per lane wherever the array starts
    // on a 16-byte boundary (the indices: 4 bytes per lane on a 4-byte boundary)
    auto aligned = [](const void *q, uintptr_t a) { return reinterpret_cast<uintptr_t>(q) % a == 0; };
    uint32_t vec = 0;
    const float *planes[4] = {p.e1, p.e2, p.e3, p.lap};
    for (int k = 0; k < 4; ++k) vec |= (uint32_t)aligned(planes[k], 16) << (SELECT_VEC_PLANE + k);
    for (int m = 0; m < n_measures; ++m) {
      vec |= (uint32_t)aligned(response + (int64_t)m * nvox, 16) << (SELECT_VEC_RESPONSE + m);
      if (index) vec |= (uint32_t)aligned(index + (int64_t)m * nvox, 4) << (SELECT_VEC_INDEX + m);
    }
    const SelectMeasures ms = select_measures(measures, n_measures, sigmas[s]);
    // booked as `mask_f64`, the row of the pointwise kernels (ife_threshold_mask's too): no other
    // kernel of this call is, so the row is the fold alone
    ProfScope ps(ctx, KK_MASK);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, p, nvox, ms, s, vec, response,
                         index);
    };
    if (s == 0) {
      if (index) launch(scale_fold_kernel<true, true>);
      else launch(scale_fold_kernel<true, false>);
    } else {
      if (index) launch(scale_fold_kernel<false, true>);
      else launch(scale_fold_kernel<false, false>);
    }
    IFE_HIP(ctx, hipGetLastError());
    return IFE_OK;
  }
};

}  // namespace

extern "C" {

int ife_scale_select(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                     const ife_volume_desc *vol, const float *sigmas, int n_sigmas,
                     const ife_scale_measure *measures, int n_measures, float *response, uint8_t *scale_index,
                     int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = features_check(ctx, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, response != nullptr,
                           IFE_PLANAR, mem)))
    return rc;
  const char *msg = "";
  int which = -1;
  if (scale_select_check(measures != nullptr, n_measures, n_sigmas, measures, &msg, &which))
    return which < 0 ? fail(ctx, IFE_E_ARG, "%s", msg) : fail(ctx, IFE_E_ARG, "measures[%d]: %s", which, msg);
  if (mem == IFE_MEM_DEVICE && reinterpret_cast<uintptr_t>(response) % 4)
    return fail(ctx, IFE_E_ARG, "response must be aligned to 4 bytes");
  const bool differential = ctx->differential != 0;
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  const size_t resp_bytes = (size_t)n_measures * n * sizeof(float), idx_bytes = scale_index ? (size_t)n_measures * n : 0;
  const void *dI, *dM;
  void *dR;
  if ((rc = stage_in(ctx, mem, image, n * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, mask, n * (mask ? dtype_size(mask_dtype) : 0), ctx->st_mask, &dM))) return rc;
  // HOST mode: both outputs in one staging area, the indices behind the responses
  if ((rc = stage_out_begin(ctx, mem, response, resp_bytes + idx_bytes, &dR))) return rc;
  uint8_t *dX = !scale_index ? nullptr : mem == IFE_MEM_HOST ? (uint8_t *)dR + resp_bytes : scale_index;
  if ((rc = reserve_scales(ctx, vol, differential))) return rc;
  if ((rc = ensure(ctx, ctx->ss_ws, n * IFE_NUM_FEATURES * sizeof(float)))) return rc;
  rc = with_types(image_dtype, dI, dM != nullptr, mask_dtype, dM, [&](auto img, auto msk) {
    using TM = std::remove_cv_t<std::remove_pointer_t<decltype(msk)>>;
    return feature_scales(ctx, img, msk, vol, sigmas, n_sigmas, differential,
                          SelectSink<TM>{msk, (float *)ctx->ss_ws.p, sigmas, measures, n_measures, (float *)dR, dX},
                          nullptr);
  });
  if (rc) return rc;
  if (mem == IFE_MEM_HOST) {
    IFE_HIP(ctx, hipMemcpyAsync(response, dR, resp_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (scale_index) IFE_HIP(ctx, hipMemcpyAsync(scale_index, dX, idx_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the call blocks in both modes
  return IFE_OK;
}

}  // extern "C"
