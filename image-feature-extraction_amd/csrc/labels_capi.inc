// labels_capi.inc -- the per-region label modes of include/ife_hip.h (ife_roi_labels,
// ife_dense_roi_labels); included at the end of ife_capi.hip behind dense_capi.inc, whose centres,
// budget, groups and x / y passes the dense form shares.

namespace {

// ignore[] and dominant into the rule the kernels read.
int label_rule(ife_ctx *ctx, const int *ignore, int n_ignore, int dominant, LabelRule *rule) {
  if (n_ignore < 0 || (n_ignore > 0 && !ignore)) return fail(ctx, IFE_E_ARG, "null pointer");
  if (dominant > 255) return fail(ctx, IFE_E_ARG, "dominant label is to large (%d, label max 255)", dominant);
  *rule = LabelRule();
  for (int i = 0; i < n_ignore; ++i) {
    if (ignore[i] < 0 || ignore[i] > 255)
      return fail(ctx, IFE_E_ARG, "Ignored label is to large (%d, label max 255)", ignore[i]);
    rule->ignore[ignore[i] >> 5] |= 1u << (ignore[i] & 31);
  }
  rule->dominant = dominant < 0 ? -1 : dominant;
  rule->fallback = 0;
  for (int l = 255; l >= 0; --l)
    if ((rule->ignore[l >> 5] >> (l & 31)) & 1u) rule->fallback = l;
  return IFE_OK;
}
bool rule_ignores(const LabelRule &r, int l) { return (r.ignore[l >> 5] >> (l & 31)) & 1u; }

int check_labels_dtype(ife_ctx *ctx, int labels_dtype) {
  if (labels_dtype != IFE_U8) return fail(ctx, IFE_E_ARG, "labels dtype must be IFE_U8");
  return IFE_OK;
}

int check_label_rois(ife_ctx *ctx, const ife_volume_desc *vol, const int64_t *rois, int64_t n_rois) {
  for (int64_t r = 0; r < n_rois; ++r) {
    const int64_t *q = rois + 6 * r;
    const bool sized = q[3] >= 1 && q[4] >= 1 && q[5] >= 1 && q[3] <= vol->nx && q[4] <= vol->ny && q[5] <= vol->nz;
    if (!sized || q[0] < 0 || q[1] < 0 || q[2] < 0 || q[0] > vol->nx - q[3] || q[1] > vol->ny - q[4] ||
        q[2] > vol->nz - q[5])
      return fail(ctx, IFE_E_ARG,
                  "region %lld [%lld, %lld, %lld][%lld, %lld, %lld] is outside of the largest possible region "
                  "[%lld, %lld, %lld] or has a size below 1", (long long)r, (long long)q[0], (long long)q[1],
                  (long long)q[2], (long long)q[3], (long long)q[4], (long long)q[5], (long long)vol->nx,
                  (long long)vol->ny, (long long)vol->nz);
    if (q[3] * q[4] > LABELS_MAX_BOX / q[5])
      return fail(ctx, IFE_E_SIZE, "region %lld holds more than 2^32-1 voxels", (long long)r);
  }
  return IFE_OK;
}

// The planes of the dense form: the labels that occur in the volume and are not ignored, ascending,
// the dominant label last (label_mode_z_kernel's `force`).  Blocks for the presence flags.
int dense_label_order(ife_ctx *ctx, const uint8_t *dL, int64_t nvox, const LabelRule &rule, uint32_t *dPresent,
                      std::vector<int> *order) {
  uint32_t present[LABEL_VALUES];
  IFE_HIP(ctx, hipMemsetAsync(dPresent, 0, sizeof present, ctx->stream));
  {
    ProfScope ps(ctx, KK_DENSE_CODE);
    const unsigned blocks = (unsigned)std::min<int64_t>((nvox + 255) / 256, 2048);
    hipLaunchKernelGGL(label_presence_kernel, dim3(blocks), dim3(256), 0, ctx->stream, dL, nvox, dPresent);
    IFE_HIP(ctx, hipGetLastError());
  }
  IFE_HIP(ctx, hipMemcpyAsync(present, dPresent, sizeof present, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  order->clear();
  for (int l = 0; l < LABEL_VALUES; ++l)
    if (present[l] && !rule_ignores(rule, l) && l != rule.dominant) order->push_back(l);
  if (rule.dominant >= 0 && present[rule.dominant]) order->push_back(rule.dominant);
  return IFE_OK;
}

// The dense passes: dOut (preset to the rule's fallback) and dBest (zeroed) take the mode of every
// region.  Scratch per group of bg labels: nvox * (1 + 3 * bg) bytes (the codes; one byte after x
// and two after y per label), bg <= 255 from the budget as dense_groups sizes the bins of one
// component.  dLut: [groups][256] bytes on the device, filled here.
int dense_label_passes(ife_ctx *ctx, const uint8_t *dL, const DenseGeom &g, const DenseCentres &cen,
                       const LabelRule &rule, const std::vector<int> &order, uint8_t *dLut, int bg, uint32_t *dBest,
                       uint8_t *dOut) {
  const size_t nvox = (size_t)g.nvox, planes = (size_t)bg;
  const int nl = (int)order.size(), ngroups = (nl + bg - 1) / bg;
  std::vector<uint8_t> lut((size_t)ngroups * LABEL_VALUES, (uint8_t)DENSE_OUTSIDE);
  for (int i = 0; i < nl; ++i) lut[(size_t)(i / bg) * LABEL_VALUES + order[i]] = (uint8_t)(i % bg);
  IFE_HIP(ctx, hipMemcpyAsync(dLut, lut.data(), lut.size(), hipMemcpyHostToDevice, ctx->stream));
  uint16_t *ys = (uint16_t *)ctx->dn_ws.p;
  uint8_t *xs = (uint8_t *)(ys + planes * nvox), *code = xs + planes * nvox;
  const int64_t nyv = g.ny - g.sy + 1, nzv = g.nz - g.sz + 1;
  const int ychunk = (int)std::min<int64_t>(std::max<int64_t>(2 * (int64_t)g.sy, 64), nyv);
  const int zchunk = (int)std::min<int64_t>(std::max<int64_t>(2 * (int64_t)g.sz, 64), nzv);
  const int nych = (int)((nyv + ychunk - 1) / ychunk), nzch = (int)((nzv + zchunk - 1) / zchunk);
  for (int k = 0; k < ngroups; ++k) {
    const int l0 = k * bg, np = std::min(bg, nl - l0);
    {
      ProfScope ps(ctx, KK_DENSE_CODE);
      const unsigned blocks = (unsigned)std::min<int64_t>((g.nvox + 255) / 256, 1 << 16);
      hipLaunchKernelGGL(label_code_kernel, dim3(blocks), dim3(256), 0, ctx->stream, dL,
                         dLut + (size_t)k * LABEL_VALUES, code, g.nvox);
    }
    {
      ProfScope ps(ctx, KK_DENSE_XY);
      const int64_t wx = (int64_t)g.gx * g.ny * g.nz, wy = (int64_t)g.gx * g.nz * nych * np;
      hipLaunchKernelGGL(dense_box_x_kernel, dim3(dense_blocks(wx)), dim3(256), 0, ctx->stream, code, g.nvox, xs, g,
                         0, np, wx);
      hipLaunchKernelGGL(dense_box_y_kernel, dim3(dense_blocks(wy)), dim3(256), 0, ctx->stream, xs, ys, g, ychunk,
                         nych, wy);
    }
    {
      ProfScope ps(ctx, KK_DENSE_Z);  // one launch per label: the stream fixes their order
      const int64_t wz = (int64_t)g.gx * nyv * nzch;
      for (int p = 0; p < np; ++p) {
        const int label = order[l0 + p];
        hipLaunchKernelGGL(label_mode_z_kernel, dim3(dense_blocks(wz)), dim3(256), 0, ctx->stream,
                           ys + (size_t)p * nvox, cen.flag, cen.seg_base, dBest, dOut, g, label,
                           label == rule.dominant ? 1 : 0, zchunk, nzch, wz);
      }
    }
    IFE_HIP(ctx, hipGetLastError());
  }
  // the tables were copied from a vector of this frame
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return IFE_OK;
}

}  // namespace

extern "C" {

// ---- tools/ExtractLabels.cxx:164-212: the mode of the label image inside every box -----------------
int ife_roi_labels(ife_ctx *ctx, const void *labels, int labels_dtype, const ife_volume_desc *vol,
                   const int64_t *rois, int64_t n_rois, const int *ignore, int n_ignore, int dominant, uint8_t *out,
                   int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if ((rc = check_labels_dtype(ctx, labels_dtype))) return rc;
  LabelRule rule;
  if ((rc = label_rule(ctx, ignore, n_ignore, dominant, &rule))) return rc;
  if (n_rois < 0) return fail(ctx, IFE_E_ARG, "negative count");
  if (n_rois == 0) return IFE_OK;
  if (!labels || !rois || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if (mem == IFE_MEM_DEVICE && reinterpret_cast<uintptr_t>(rois) % 8)
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  if (mem == IFE_MEM_HOST && (rc = check_label_rois(ctx, vol, rois, n_rois))) return rc;
  const size_t nvox = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dL, *dR;
  void *dO;
  if ((rc = stage_in(ctx, mem, labels, nvox, ctx->st_img, &dL))) return rc;
  if ((rc = stage_in(ctx, mem, rois, (size_t)n_rois * 48, ctx->st_aux, &dR))) return rc;
  if (mem == IFE_MEM_DEVICE) {  // the boxes are checked where they are, before anything reads through them
    if ((rc = ensure(ctx, ctx->st_mask, 16))) return rc;
    int bad = 0;
    IFE_HIP(ctx, hipMemsetAsync(ctx->st_mask.p, 0, 4, ctx->stream));
    {
      ProfScope ps(ctx, KK_HIST);
      hipLaunchKernelGGL(roi_check_kernel, dim3((unsigned)std::min<int64_t>((n_rois + 255) / 256, 2048)), dim3(256), 0,
                         ctx->stream, (const int64_t *)dR, n_rois, vol->nx, vol->ny, vol->nz, (int *)ctx->st_mask.p);
      IFE_HIP(ctx, hipGetLastError());
    }
    IFE_HIP(ctx, hipMemcpyAsync(&bad, ctx->st_mask.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad)
      return fail(ctx, IFE_E_ARG, "a region is outside of the largest possible region [%lld, %lld, %lld], has a "
                  "size below 1 or holds more than 2^32-1 voxels", (long long)vol->nx, (long long)vol->ny,
                  (long long)vol->nz);
  }
  if ((rc = stage_out_begin(ctx, mem, out, (size_t)n_rois, &dO))) return rc;
  {
    ProfScope ps(ctx, KK_HIST);
    // n_rois is 64 bits wide and the grid is not: at most LABELS_GRID_CAP workgroups, which loop
    const unsigned blocks = (unsigned)std::min<int64_t>(n_rois, LABELS_GRID_CAP);
    hipLaunchKernelGGL(roi_labels_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const uint8_t *)dL,
                       (const int64_t *)dR, n_rois, vol->nx, vol->ny, rule, (uint8_t *)dO);
    IFE_HIP(ctx, hipGetLastError());
  }
  if (mem == IFE_MEM_DEVICE) {  // the call blocks in both modes
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IFE_OK;
  }
  return stage_out_end(ctx, mem, out, (size_t)n_rois);
}

// ---- the labels ife_roi_labels gives for the dense boxes, without the boxes ----------------------------
int ife_dense_roi_labels(ife_ctx *ctx, const void *labels, int labels_dtype, const void *gen_mask, int gen_mask_dtype,
                         const ife_volume_desc *vol, const int64_t size[3], const int *ignore, int n_ignore,
                         int dominant, uint8_t *out, int64_t capacity, int64_t *n_rois, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if ((rc = check_labels_dtype(ctx, labels_dtype))) return rc;
  if (!labels || !n_rois) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mask_dtype(ctx, gen_mask, gen_mask_dtype, false))) return rc;
  LabelRule rule;
  if ((rc = label_rule(ctx, ignore, n_ignore, dominant, &rule))) return rc;
  if (out && capacity < 0) return fail(ctx, IFE_E_ARG, "negative capacity");
  if (mem == IFE_MEM_DEVICE && reinterpret_cast<uintptr_t>(gen_mask) % dtype_size(gen_mask_dtype))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  DenseGeom g;
  bool empty = false;
  if ((rc = dense_geom(ctx, vol, size, true, &g, &empty))) return rc;
  *n_rois = 0;
  if (empty) return IFE_OK;
  const size_t nvox = (size_t)g.nvox;
  const void *dG, *dL;
  if ((rc = stage_in(ctx, mem, gen_mask, nvox * dtype_size(gen_mask_dtype), ctx->st_mask, &dG))) return rc;
  DenseCentres cen;  // without an array for the labels the call counts only
  rc = dense_centres(ctx, dG, gen_mask_dtype, g, ctx->dn_centres, out ? capacity : INT64_MAX, n_rois, &cen);
  if (rc || !out || cen.n == 0) return rc;
  if ((rc = stage_in(ctx, mem, labels, nvox, ctx->st_img, &dL))) return rc;
  void *dO;
  if ((rc = stage_out_begin(ctx, mem, out, (size_t)cen.n, &dO))) return rc;
  const bool settled = rule.dominant >= 0 && rule_ignores(rule, rule.dominant);  // clause 1 everywhere
  IFE_HIP(ctx, hipMemsetAsync(dO, settled ? rule.dominant : rule.fallback, (size_t)cen.n, ctx->stream));
  if (!settled) {
    // st_aux: the presence flags, behind them the code tables of the groups
    if ((rc = ensure(ctx, ctx->st_aux, 1024 + (size_t)LABEL_VALUES * LABEL_VALUES))) return rc;
    std::vector<int> order;
    if ((rc = dense_label_order(ctx, (const uint8_t *)dL, g.nvox, rule, (uint32_t *)ctx->st_aux.p, &order))) return rc;
    if (!order.empty()) {
      size_t budget;
      if ((rc = dense_budget(ctx, ctx->dn_ws.cap, &budget))) return rc;
      int cg, bg;
      if ((rc = dense_groups(ctx, budget, nvox, 1, std::min<int>((int)order.size(), DENSE_OUTSIDE), 1, &cg, &bg)))
        return rc;
      if ((rc = ensure(ctx, ctx->dn_ws, nvox * (3 * (size_t)bg + 1)))) return rc;
      if ((rc = ensure(ctx, ctx->dn_feat, (size_t)cen.n * 4))) return rc;  // the best count of every region
      IFE_HIP(ctx, hipMemsetAsync(ctx->dn_feat.p, 0, (size_t)cen.n * 4, ctx->stream));
      if ((rc = dense_label_passes(ctx, (const uint8_t *)dL, g, cen, rule, order, (uint8_t *)ctx->st_aux.p + 1024, bg,
                                   (uint32_t *)ctx->dn_feat.p, (uint8_t *)dO)))
        return rc;
    }
  }
  if (mem == IFE_MEM_DEVICE) {
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IFE_OK;
  }
  return stage_out_end(ctx, mem, out, (size_t)cen.n);
}

}  // extern "C"
