// dense_capi.inc -- the dense bag entry points of include/ife_hip.h (ife_dense_rois,
// ife_dense_roi_histograms, ife_bag_image_dense, ife_bag_dense_stream_begin / _next / _end);
// included at the end of ife_capi.hip (shares its context, staging and profiling helpers, and
// clamp01 / the scans of stats_capi.inc).

namespace {

unsigned dense_blocks(int64_t nwaves) {  // 4 waves per workgroup, grid-stride beyond
  return (unsigned)std::min<int64_t>(std::max<int64_t>((nwaves + 3) / 4, 1), 1 << 18);
}

// size[] and the volume into a DenseGeom.  *empty: a box larger than the volume, no region (not an
// error).  with_counters: the box must fit the counter widths of the three passes.
int dense_geom(ife_ctx *ctx, const ife_volume_desc *vol, const int64_t *size, bool with_counters, DenseGeom *g,
               bool *empty) {
  if (!size) return fail(ctx, IFE_E_ARG, "null pointer");
  if (size[0] < 1 || size[1] < 1 || size[2] < 1)
    return fail(ctx, IFE_E_ARG, "the box size must be at least 1 along every axis (got %lld x %lld x %lld)",
                (long long)size[0], (long long)size[1], (long long)size[2]);
  if (with_counters && (size[0] > DENSE_MAX_SX || size[1] > DENSE_MAX_SXY / size[0] ||
                        size[2] > DENSE_MAX_SXYZ / (size[0] * size[1])))
    return fail(ctx, IFE_E_SIZE,
                "box %lld x %lld x %lld does not fit the counters: sx <= %lld, sx*sy <= %lld, sx*sy*sz <= %lld",
                (long long)size[0], (long long)size[1], (long long)size[2], (long long)DENSE_MAX_SX,
                (long long)DENSE_MAX_SXY, (long long)DENSE_MAX_SXYZ);
  *empty = size[0] > vol->nx || size[1] > vol->ny || size[2] > vol->nz;
  if (*empty) return IFE_OK;
  g->nx = vol->nx; g->ny = vol->ny; g->nz = vol->nz;
  g->nvox = vol->nx * vol->ny * vol->nz;
  g->sx = (int)size[0]; g->sy = (int)size[1]; g->sz = (int)size[2];
  g->hx = g->sx / 2; g->hy = g->sy / 2; g->hz = g->sz / 2;
  g->gx = (int)((vol->nx + 63) / 64);
  // regions are numbered in 32 bits (the scan of the segment counts)
  if (g->nvox >= (int64_t)1 << 32 || (int64_t)g->gx * vol->ny * vol->nz >= (int64_t)1 << 31)
    return fail(ctx, IFE_E_SIZE, "volume too large for 32-bit region numbers");
  return IFE_OK;
}

struct DenseCentres {
  const uint8_t *flag;      // [nvox] 1 = centre
  const uint32_t *seg_base; // [nseg] number of the first centre of every row segment
  int64_t nseg, n;          // n: number of centres
};

// Flags and numbers the centres of `gen` (device) into `buf` (ctx->dn_centres, or the stream's
// own); blocks for the count, which goes to *n_rois as well.  More than `capacity` is an error.
int dense_centres(ife_ctx *ctx, const void *dG, int gen_dtype, const DenseGeom &g, DevBuf &buf, int64_t capacity,
                  int64_t *n_rois, DenseCentres *out) {
  const int64_t nseg = (int64_t)g.gx * g.ny * g.nz;
  int rc = ensure(ctx, buf, seg_scan_bytes(nseg) + (size_t)g.nvox);  // the flags stand behind the scan's own
  if (rc) return rc;
  uint32_t *segs = seg_counts(buf);
  uint8_t *flag = (uint8_t *)buf.p + seg_scan_bytes(nseg);
  {
    ProfScope ps(ctx, KK_DENSE_CODE);
    with_mask_type(true, gen_dtype, dG, [&](auto gen) -> int {
      using TM = std::remove_cv_t<std::remove_pointer_t<decltype(gen)>>;
      hipLaunchKernelGGL(dense_centre_kernel<TM>, dim3(dense_blocks(nseg)), dim3(256), 0, ctx->stream, gen, flag,
                         segs, g, nseg);
      return IFE_OK;
    });
    if ((rc = seg_scan(ctx, buf, nseg))) return rc;
  }
  out->flag = flag;
  out->seg_base = segs;
  out->nseg = nseg;
  if ((rc = scan_total(ctx, buf, &out->n))) return rc;
  *n_rois = out->n;
  if (out->n > capacity)
    return fail(ctx, IFE_E_SIZE, "%lld regions, the output holds %lld", (long long)out->n, (long long)capacity);
  return IFE_OK;
}

// Bytes the caller may spend on scratch: IFE_OPT_DENSE_SCRATCH_MB when set, else four fifths of
// the free device memory, counting what `held` already holds (it is regrown, not added to).
int dense_budget(ife_ctx *ctx, size_t held, size_t *budget) {
  if (ctx->dense_scratch_mb > 0) {
    *budget = (size_t)ctx->dense_scratch_mb << 20;
    return IFE_OK;
  }
  size_t free_b = 0, total_b = 0;
  IFE_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
  *budget = (free_b + held) / 5 * 4;
  return IFE_OK;
}

// Components and bins the box passes take at a time: whole components (cg of them, all nb bins)
// while they fit into `budget`, else one component and as many bins (bg) as fit.  Scratch per
// group: nvox * cg * (code_bytes + 3 * bg) bytes (one byte after x and two after y per plane, and
// code_bytes = 1 where the codes of the group live in the scratch too, 0 where they exist already).
int dense_groups(ife_ctx *ctx, size_t budget, size_t nvox, int ncomp, int nb, int code_bytes, int *cg, int *bg) {
  *cg = (int)std::min<size_t>({(size_t)ncomp, budget / (nvox * (code_bytes + 3 * (size_t)nb)), (size_t)1024});
  *bg = nb;
  if (*cg < 1) {
    *cg = 1;
    *bg = budget > code_bytes * nvox ? (int)std::min<size_t>((budget - code_bytes * nvox) / (3 * nvox), (size_t)nb) : 0;
    if (*bg < 1)
      return fail(ctx, IFE_E_NOMEM, "the dense box counts need %zu bytes of scratch for one bin, %zu are available",
                  (3 + code_bytes) * nvox, budget);
  }
  return IFE_OK;
}

// Bin codes of components [c0, c0 + nc) of one feature volume (device): code[c - c0][voxel].
int dense_code(ife_ctx *ctx, const float *dF, int64_t comp_stride, int64_t vox_stride, int c0, int nc, const void *dM,
               int mask_dtype, int64_t nvox, const float *dEdges, int n_edges, uint8_t *code) {
  ProfScope ps(ctx, KK_DENSE_CODE);
  const dim3 grid((unsigned)std::min<int64_t>((nvox + 255) / 256, 1 << 16), (unsigned)nc);
  return with_mask_type(true, mask_dtype, dM, [&](auto msk) -> int {
    using TM = std::remove_cv_t<std::remove_pointer_t<decltype(msk)>>;
    hipLaunchKernelGGL(dense_code_kernel<TM>, grid, dim3(256), 0, ctx->stream, dF, msk, dEdges, code, nvox,
                       comp_stride, vox_stride, c0, n_edges);
    IFE_HIP(ctx, hipGetLastError());
    return IFE_OK;
  });
}

// Where the z pass stores: counts[(number - row0) * row_stride + column * col_stride].
struct DenseOut {
  uint32_t *counts;
  int64_t row0, row_stride, col_stride;
};

// The box passes over nc components whose codes are at code[c * code_stride + voxel of g], the nb
// bins in groups of bg; the counts go to columns col0 + c * nb + bin of `out`.  g may be a block
// of planes of a larger volume: code, flag and seg_base then point at the block's first plane.
// scratch: ys [planes][g.nvox] two bytes, then xs [planes][g.nvox] one byte, planes >= nc * bg.
int dense_box_passes(ife_ctx *ctx, const uint8_t *code, int64_t code_stride, int nc, const DenseGeom &g,
                     const uint8_t *flag, const uint32_t *seg_base, void *scratch, size_t planes, int bg, int nb,
                     const DenseOut &out, int64_t col0) {
  uint16_t *ys = (uint16_t *)scratch;
  uint8_t *xs = (uint8_t *)(ys + planes * (size_t)g.nvox);
  // marching passes: a wave covers `chunk` outputs after a start-up of (window - 1) reads
  const int64_t nyv = g.ny - g.sy + 1, nzv = g.nz - g.sz + 1;
  const int ychunk = (int)std::min<int64_t>(std::max<int64_t>(2 * (int64_t)g.sy, 64), nyv);
  const int zchunk = (int)std::min<int64_t>(std::max<int64_t>(2 * (int64_t)g.sz, 64), nzv);
  const int nych = (int)((nyv + ychunk - 1) / ychunk), nzch = (int)((nzv + zchunk - 1) / zchunk);
  for (int b0 = 0; b0 < nb; b0 += bg) {
    const int nbins = std::min(bg, nb - b0);
    const int64_t np = (int64_t)nc * nbins;
    {
      ProfScope ps(ctx, KK_DENSE_XY);
      const int64_t wx = (int64_t)g.gx * g.ny * g.nz * nc, wy = (int64_t)g.gx * g.nz * nych * np;
      hipLaunchKernelGGL(dense_box_x_kernel, dim3(dense_blocks(wx)), dim3(256), 0, ctx->stream, code, code_stride,
                         xs, g, b0, nbins, wx);
      hipLaunchKernelGGL(dense_box_y_kernel, dim3(dense_blocks(wy)), dim3(256), 0, ctx->stream, xs, ys, g, ychunk,
                         nych, wy);
    }
    {
      ProfScope ps(ctx, KK_DENSE_Z);
      const int64_t wz = (int64_t)g.gx * nyv * nzch * np;
      hipLaunchKernelGGL(dense_box_z_kernel, dim3(dense_blocks(wz)), dim3(256), 0, ctx->stream, ys, flag, seg_base,
                         out.counts, g, nbins, nb, out.row0, out.row_stride, out.col_stride, col0 + b0, zchunk, nzch,
                         wz);
    }
    IFE_HIP(ctx, hipGetLastError());
  }
  return IFE_OK;
}

// The box counts of components [0, ncomp) of one feature volume (device), written at the centres:
// dCounts[number * row_words + col0 + c * (n_edges + 1) + bin].  dEdges: [ncomp][n_edges], device.
// Scratch per group of cg components and bg bins: nvox * cg * (1 + 3 * bg) bytes (codes; one byte
// after x and two after y per plane), sized from `budget`.
int dense_count(ife_ctx *ctx, const float *dF, int layout, int ncomp, const void *dM, int mask_dtype,
                const DenseGeom &g, const DenseCentres &cen, const float *dEdges, int n_edges, uint32_t *dCounts,
                int64_t row_words, int64_t col0, size_t budget) {
  const int nb = n_edges + 1;
  const size_t nvox = (size_t)g.nvox;
  int cg, bg;
  int rc = dense_groups(ctx, budget, nvox, ncomp, nb, 1, &cg, &bg);
  if (rc) return rc;
  const size_t planes = (size_t)cg * bg;
  if ((rc = ensure(ctx, ctx->dn_ws, nvox * (3 * planes + cg)))) return rc;
  uint8_t *code = (uint8_t *)ctx->dn_ws.p + 3 * planes * nvox;  // behind ys and xs: [cg][nvox]
  const int64_t comp_stride = layout == IFE_PLANAR ? g.nvox : 1, vox_stride = layout == IFE_PLANAR ? 1 : ncomp;
  const DenseOut out = {dCounts, 0, row_words, 1};
  for (int c0 = 0; c0 < ncomp; c0 += cg) {
    const int nc = std::min(cg, ncomp - c0);
    if ((rc = dense_code(ctx, dF, comp_stride, vox_stride, c0, nc, dM, mask_dtype, g.nvox, dEdges, n_edges, code)))
      return rc;
    if ((rc = dense_box_passes(ctx, code, g.nvox, nc, g, cen.flag, cen.seg_base, ctx->dn_ws.p, planes, bg, nb, out,
                               col0 + (int64_t)c0 * nb)))
      return rc;
  }
  return IFE_OK;
}

// Arguments shared by the two histogram calls (everything but their inputs).
int dense_hist_check(ife_ctx *ctx, const void *mask, int mask_dtype, const void *gen_mask, int gen_mask_dtype,
                     const float *edges, int n_edges, const void *counts, int64_t capacity,
                     const int64_t *n_rois, int mem) {
  int rc = check_mem(ctx, mem);
  if (rc) return rc;
  if (!edges || !counts || !n_rois) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, false))) return rc;
  if ((rc = check_mask_dtype(ctx, gen_mask, gen_mask_dtype, true))) return rc;
  if (n_edges < 1 || n_edges > DENSE_MAX_EDGES)
    return fail(ctx, IFE_E_ARG, "between 1 and %d edges per histogram (one byte per voxel holds the bin)",
                DENSE_MAX_EDGES);
  if (capacity < 0) return fail(ctx, IFE_E_ARG, "negative capacity");
  if (mem == IFE_MEM_DEVICE &&
      (reinterpret_cast<uintptr_t>(mask) % dtype_size(mask_dtype) ||
       (gen_mask && reinterpret_cast<uintptr_t>(gen_mask) % dtype_size(gen_mask_dtype))))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  return IFE_OK;
}

struct DenseInputs {       // the inputs of the histogram calls on the device
  const void *mask, *gen;  // gen: the mask that generates the regions, with its dtype
  int gen_dtype;
  const float *edges;
};

// Stages the mask (st_mask) and, into st_aux, the generating mask (HOST mode) and the edges behind
// it.  edges_mem: where the caller's edges are; IFE_MEM_DEVICE (so is `mem` then) leaves them in place.
int dense_stage(ife_ctx *ctx, int mem, const void *mask, int mask_dtype, const void *gen_mask, int gen_mask_dtype,
                size_t nvox, const float *edges, size_t ebytes, int edges_mem, DenseInputs *in) {
  const size_t gbytes = gen_mask ? nvox * dtype_size(gen_mask_dtype) : 0, off_e = (gbytes + 15) / 16 * 16;
  const void *dG = gen_mask;
  int rc;
  if ((rc = stage_in(ctx, mem, mask, nvox * dtype_size(mask_dtype), ctx->st_mask, &in->mask))) return rc;
  in->edges = edges;
  if (edges_mem == IFE_MEM_HOST) {
    if ((rc = ensure(ctx, ctx->st_aux, off_e + ebytes))) return rc;
    if (gen_mask && mem == IFE_MEM_HOST) {
      IFE_HIP(ctx, hipMemcpyAsync(ctx->st_aux.p, gen_mask, gbytes, hipMemcpyHostToDevice, ctx->stream));
      dG = ctx->st_aux.p;
    }
    in->edges = (const float *)((char *)ctx->st_aux.p + off_e);
    IFE_HIP(ctx, hipMemcpyAsync((char *)ctx->st_aux.p + off_e, edges, ebytes, hipMemcpyHostToDevice, ctx->stream));
  }
  in->gen = dG ? dG : in->mask;
  in->gen_dtype = dG ? gen_mask_dtype : mask_dtype;
  return IFE_OK;
}

// Scales in groups: the clamped labels and the planar features of `sg` scales (32 bytes per voxel
// and scale) live in dn_feat, labels first, and take at most `budget` (but one scale at least).
struct DenseScalePlan { int sg; size_t off_f, fbytes; };
DenseScalePlan dense_scale_plan(size_t budget, size_t nvox, int n_sigmas) {
  const size_t scale_bytes = nvox * IFE_NUM_FEATURES * 4, off_f = (nvox + 15) / 16 * 16;
  const int sg = (int)std::min<size_t>(std::max<size_t>(budget / scale_bytes, 1), (size_t)n_sigmas);
  return {sg, off_f, off_f + (size_t)sg * scale_bytes};
}

// Clamps the labels once, then the features of every group of plan.sg scales into dn_feat and
// each_scale(scale, its planar features, the clamped labels) for every scale of the group.
template <typename F>
int dense_scale_loop(ife_ctx *ctx, const void *dI, int image_dtype, const void *dM, int mask_dtype,
                     const ife_volume_desc *vol, const float *sigmas, int n_sigmas, const DenseScalePlan &plan,
                     F &&each_scale) {
  const size_t nvox = (size_t)(vol->nx * vol->ny * vol->nz);
  int rc = ensure(ctx, ctx->dn_feat, plan.fbytes);
  if (rc) return rc;
  uint8_t *clamp = (uint8_t *)ctx->dn_feat.p;
  float *feat = (float *)((char *)ctx->dn_feat.p + plan.off_f);
  if ((rc = launch_clamp01(ctx, dM, mask_dtype, clamp, (int64_t)nvox))) return rc;
  for (int s0 = 0; s0 < n_sigmas; s0 += plan.sg) {
    const int ns = std::min(plan.sg, n_sigmas - s0);
    if ((rc = feature_volumes(ctx, dI, image_dtype, clamp, IFE_U8, vol, sigmas + s0, ns, feat, IFE_PLANAR, false)))
      return rc;
    for (int i = 0; i < ns; ++i)
      if ((rc = each_scale(s0 + i, feat + (size_t)i * nvox * IFE_NUM_FEATURES, clamp))) return rc;
  }
  return IFE_OK;
}

// IFE_OPT_DIFFERENTIAL: no feature volume.  The clamped labels stand at the start of dn_feat
// (`fbytes` of it are ensured: the caller may keep more behind them); the scale loop hands the
// twenty fields of every scale to a CodeSink (scales_capi.inc) with the caller's code_of and
// each_scale.  dEdges: [n_sigmas * 8][n_edges], device.
template <typename C, typename F>
int dense_code_scales(ife_ctx *ctx, const void *dI, int image_dtype, const void *dM, int mask_dtype,
                      const ife_volume_desc *vol, const float *sigmas, int n_sigmas, const float *dEdges, int n_edges,
                      size_t fbytes, C code_of, F each_scale) {
  int rc = ensure(ctx, ctx->dn_feat, fbytes);
  if (rc) return rc;
  uint8_t *clamp = (uint8_t *)ctx->dn_feat.p;
  if ((rc = launch_clamp01(ctx, dM, mask_dtype, clamp, vol->nx * vol->ny * vol->nz))) return rc;
  return with_types(image_dtype, dI, true, IFE_U8, clamp, [&](auto img, auto cm) {
    return feature_scales(ctx, img, cm, vol, sigmas, n_sigmas, true,
                          CodeSink<C, F>{clamp, dEdges, n_edges, code_of, each_scale}, nullptr);
  });
}

}  // namespace

extern "C" {

// ---- DenseROIGenerator<TMask>::generate (include/ife/ROI/DenseROIGenerator.hxx:24-46) ----------
int ife_dense_rois(ife_ctx *ctx, const void *gen_mask, int gen_mask_dtype, const ife_volume_desc *vol,
                   const int64_t size[3], int64_t *n_rois, int64_t *rois, int64_t capacity, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!n_rois) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mask_dtype(ctx, gen_mask, gen_mask_dtype, false))) return rc;
  if (rois && capacity < 0) return fail(ctx, IFE_E_ARG, "negative capacity");
  if (mem == IFE_MEM_DEVICE && (reinterpret_cast<uintptr_t>(gen_mask) % dtype_size(gen_mask_dtype) ||
                                reinterpret_cast<uintptr_t>(rois) % 8))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  DenseGeom g;
  bool empty = false;
  if ((rc = dense_geom(ctx, vol, size, false, &g, &empty))) return rc;
  *n_rois = 0;
  if (empty) return IFE_OK;
  const void *dG;
  if ((rc = stage_in(ctx, mem, gen_mask, (size_t)g.nvox * dtype_size(gen_mask_dtype), ctx->st_mask, &dG))) return rc;
  DenseCentres cen;  // without an array for the boxes the call counts only
  rc = dense_centres(ctx, dG, gen_mask_dtype, g, ctx->dn_centres, rois ? capacity : INT64_MAX, n_rois, &cen);
  if (rc || !rois || cen.n == 0) return rc;
  void *dR;
  if ((rc = stage_out_begin(ctx, mem, rois, (size_t)cen.n * 48, &dR))) return rc;
  {
    ProfScope ps(ctx, KK_DENSE_CODE);
    hipLaunchKernelGGL(dense_boxes_kernel, dim3(dense_blocks(cen.nseg)), dim3(256), 0, ctx->stream, cen.flag,
                       cen.seg_base, (int64_t *)dR, g, cen.nseg);
    IFE_HIP(ctx, hipGetLastError());
  }
  if (mem == IFE_MEM_DEVICE) {  // the call blocks in both modes
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IFE_OK;
  }
  return stage_out_end(ctx, mem, rois, (size_t)cen.n * 48);
}

// ---- the rows of ife_roi_histograms for the dense boxes, without the boxes -----------------------
int ife_dense_roi_histograms(ife_ctx *ctx, const float *features, int layout, int ncomp, const void *mask,
                             int mask_dtype, const void *gen_mask, int gen_mask_dtype,
                             const ife_volume_desc *vol, const int64_t size[3], const float *edges, int n_edges,
                             uint32_t *counts, int64_t capacity, int64_t *n_rois, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_layout_mem(ctx, layout, mem))) return rc;
  if (!features) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = dense_hist_check(ctx, mask, mask_dtype, gen_mask, gen_mask_dtype, edges, n_edges, counts, capacity,
                             n_rois, mem)))
    return rc;
  if (ncomp < 1 || ncomp > 65536) return fail(ctx, IFE_E_ARG, "between 1 and 65536 components");
  if (mem == IFE_MEM_DEVICE && (reinterpret_cast<uintptr_t>(features) % 4 || reinterpret_cast<uintptr_t>(edges) % 4 ||
                                reinterpret_cast<uintptr_t>(counts) % 4))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  DenseGeom g;
  bool empty = false;
  if ((rc = dense_geom(ctx, vol, size, true, &g, &empty))) return rc;
  *n_rois = 0;
  if (empty) return IFE_OK;
  const size_t nvox = (size_t)g.nvox;
  DenseInputs in;  // in DEVICE mode the caller's edges are read in place
  if ((rc = dense_stage(ctx, mem, mask, mask_dtype, gen_mask, gen_mask_dtype, nvox, edges,
                        (size_t)ncomp * n_edges * 4, mem, &in)))
    return rc;
  DenseCentres cen;
  rc = dense_centres(ctx, in.gen, in.gen_dtype, g, ctx->dn_centres, capacity, n_rois, &cen);
  if (rc || cen.n == 0) return rc;
  const void *dF;
  if ((rc = stage_in(ctx, mem, features, nvox * ncomp * 4, ctx->st_img, &dF))) return rc;
  const size_t cbytes = (size_t)cen.n * ncomp * (n_edges + 1) * 4;
  void *dC;
  if ((rc = stage_out_begin(ctx, mem, counts, cbytes, &dC))) return rc;
  size_t budget;
  if ((rc = dense_budget(ctx, ctx->dn_ws.cap, &budget))) return rc;
  if ((rc = dense_count(ctx, (const float *)dF, layout, ncomp, in.mask, mask_dtype, g, cen, in.edges, n_edges,
                        (uint32_t *)dC, (int64_t)ncomp * (n_edges + 1), 0, budget)))
    return rc;
  if (mem == IFE_MEM_DEVICE) {
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IFE_OK;
  }
  return stage_out_end(ctx, mem, counts, cbytes);
}

// ---- one image of MakeBagDense: ife_bag_image with the dense rule in place of the box list ---------
int ife_bag_image_dense(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                        const void *gen_mask, int gen_mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                        int n_sigmas, const int64_t size[3], const float *edges, int n_edges, uint32_t *counts,
                        int64_t capacity, int64_t *n_rois, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, true))) return rc;
  if (!image || !sigmas) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = dense_hist_check(ctx, mask, mask_dtype, gen_mask, gen_mask_dtype, edges, n_edges, counts, capacity,
                             n_rois, mem)))
    return rc;
  if ((rc = check_sigmas(ctx, sigmas, n_sigmas))) return rc;
  if ((rc = check_image_dtype(ctx, image_dtype))) return rc;
  DenseGeom g;
  bool empty = false;
  if ((rc = dense_geom(ctx, vol, size, true, &g, &empty))) return rc;
  *n_rois = 0;
  if (empty) return IFE_OK;
  const size_t nvox = (size_t)g.nvox;
  const int ncol = n_sigmas * IFE_NUM_FEATURES, nb = n_edges + 1;
  DenseInputs in;  // the edges are a host array in both modes
  if ((rc = dense_stage(ctx, mem, mask, mask_dtype, gen_mask, gen_mask_dtype, nvox, edges,
                        (size_t)ncol * n_edges * 4, IFE_MEM_HOST, &in)))
    return rc;
  // the image goes up only once there are regions to count, and not too many
  DenseCentres cen;
  rc = dense_centres(ctx, in.gen, in.gen_dtype, g, ctx->dn_centres, capacity, n_rois, &cen);
  if (rc || cen.n == 0) return rc;
  const void *dI;
  if ((rc = stage_in(ctx, mem, image, nvox * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  const size_t cbytes = (size_t)cen.n * ncol * nb * 4;
  if ((rc = ensure(ctx, ctx->st_out, cbytes))) return rc;
  // IFE_OPT_DIFFERENTIAL: the jet workspace first (outside the bound, as the finite-difference
  // workspace is, which the feature call grows), so that the free memory is what is left
  const bool differential = ctx->differential != 0;
  if (differential && (rc = reserve_scales(ctx, vol, true))) return rc;
  size_t budget;
  if ((rc = dense_budget(ctx, ctx->dn_ws.cap + ctx->dn_feat.cap, &budget))) return rc;
  if (differential) {
    // labels and the codes of one scale (always taken), and the box passes, which find their codes
    // in place, get the rest
    const size_t off_c = (nvox + 15) / 16 * 16, fbytes = off_c + nvox * IFE_NUM_FEATURES;
    int cg, bg;
    if ((rc = dense_groups(ctx, budget > fbytes ? budget - fbytes : 0, nvox, IFE_NUM_FEATURES, nb, 0, &cg, &bg)))
      return rc;
    const size_t planes = (size_t)cg * bg;
    if ((rc = ensure(ctx, ctx->dn_ws, 3 * planes * nvox))) return rc;
    const DenseOut out = {(uint32_t *)ctx->st_out.p, 0, (int64_t)ncol * nb, 1};
    auto box_scale = [&](int s, const uint8_t *code, const uint8_t *) {
      int r = IFE_OK;
      for (int c0 = 0; c0 < IFE_NUM_FEATURES && !r; c0 += cg)
        r = dense_box_passes(ctx, code + (size_t)c0 * nvox, g.nvox, std::min(cg, IFE_NUM_FEATURES - c0), g, cen.flag,
                             cen.seg_base, ctx->dn_ws.p, planes, bg, nb, out,
                             ((int64_t)s * IFE_NUM_FEATURES + c0) * nb);
      return r;
    };
    rc = dense_code_scales(ctx, dI, image_dtype, in.mask, mask_dtype, vol, sigmas, n_sigmas, in.edges, n_edges, fbytes,
                           [&](int) { return (uint8_t *)ctx->dn_feat.p + off_c; }, box_scale);
  } else {
    // at most half of the budget for the features of a group of scales, the box counts get the rest
    const DenseScalePlan plan = dense_scale_plan(budget / 2, nvox, n_sigmas);
    const size_t rest = budget > plan.fbytes ? budget - plan.fbytes : 0;
    auto count_scale = [&](int s, const float *feat, const uint8_t *clamp) {  // into its block of columns
      return dense_count(ctx, feat, IFE_PLANAR, IFE_NUM_FEATURES, clamp, IFE_U8, g, cen,
                         in.edges + (size_t)s * IFE_NUM_FEATURES * n_edges, n_edges, (uint32_t *)ctx->st_out.p,
                         (int64_t)ncol * nb, (int64_t)s * IFE_NUM_FEATURES * nb, rest);
    };
    rc = dense_scale_loop(ctx, dI, image_dtype, in.mask, mask_dtype, vol, sigmas, n_sigmas, plan, count_scale);
  }
  if (rc) return rc;
  IFE_HIP(ctx, hipMemcpyAsync(counts, ctx->st_out.p, cbytes, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return IFE_OK;
}

}  // extern "C"

// ---- the dense bag as a stream of row blocks --------------------------------------------------------
// The bin codes of all scales stay on the device (one byte per voxel and column); the regions of a
// block of centre planes (dense_plan.hpp) are counted from them into a planar block buffer,
// turned into row-major counts or frequencies (dense_freq_kernel) and copied out on a copy stream
// while the next block is counted.  Nothing as large as the bag exists anywhere.
namespace {

void dense_stream_release(ife_ctx *ctx) {
  auto &ds = ctx->ds;
  if (ds.open) {  // kernels or a copy of a block may still be in flight
    (void)hipStreamSynchronize(ctx->stream);
    if (ds.copy) (void)hipStreamSynchronize(ds.copy);
  }
  for (auto e : ds.done)
    if (e) (void)hipEventDestroy(e);
  // a fresh stream state frees every buffer of the old one; the copy stream lives on with the context
  const hipStream_t copy = ds.copy;
  ds = ife_ctx::DenseStream();
  ds.copy = copy;
}

// Enqueues block k: the box passes from the codes of its planes into the planar buffer, then the
// row-major block into rows[k % 2], and the event that says so.  Does not wait.
int dense_stream_count(ife_ctx *ctx, size_t k) {
  auto &ds = ctx->ds;
  const DenseBlock &b = ds.blocks[k];
  const DenseGeom &g = ds.g;
  const int64_t plane = g.nx * g.ny, z0 = b.zc0 - g.hz;  // z0: first plane of codes the block reads
  DenseGeom gb = g;
  gb.nz = b.zc1 - b.zc0 + g.sz - 1;
  gb.nvox = plane * gb.nz;
  const DenseOut out = {(uint32_t *)ds.planar.p, b.row0, 1, ds.ld};
  int rc;
  for (int c0 = 0; c0 < ds.ncol; c0 += ds.cg) {
    const int nc = std::min(ds.cg, ds.ncol - c0);
    if ((rc = dense_box_passes(ctx, (const uint8_t *)ds.codes.p + (size_t)c0 * g.nvox + z0 * plane, g.nvox, nc, gb,
                               ds.flag + z0 * plane, ds.seg_base + (int64_t)g.gx * g.ny * z0, ds.ws.p,
                               (size_t)ds.cg * ds.bg, ds.bg, ds.nb, out, (int64_t)c0 * ds.nb)))
      return rc;
  }
  {
    ProfScope ps(ctx, KK_DENSE_Z);  // the kernel-time table is full: the transposition counts as the z pass's store
    // rows x whole histograms per tile: 64 rows while one histogram fits beside them, else 32
    const int tr_log2 = ds.nb * 65 <= DENSE_FREQ_LDS_WORDS ? 6 : 5, tr = 1 << tr_log2;
    const int hists = std::max(1, std::min(ds.ncol, DENSE_FREQ_LDS_WORDS / (tr + 1) / ds.nb));
    const dim3 grid((unsigned)((b.n_rows + tr - 1) / tr), (unsigned)std::min((ds.ncol + hists - 1) / hists, 65535));
    if (ds.values == IFE_BAG_FREQUENCIES)
      hipLaunchKernelGGL(dense_freq_kernel<true>, grid, dim3(256), 0, ctx->stream, (const uint32_t *)ds.planar.p,
                         (uint32_t *)ds.rows[k % 2].p, b.n_rows, ds.ld, ds.ncol, ds.nb, hists, tr_log2);
    else
      hipLaunchKernelGGL(dense_freq_kernel<false>, grid, dim3(256), 0, ctx->stream, (const uint32_t *)ds.planar.p,
                         (uint32_t *)ds.rows[k % 2].p, b.n_rows, ds.ld, ds.ncol, ds.nb, hists, tr_log2);
    IFE_HIP(ctx, hipGetLastError());
  }
  IFE_HIP(ctx, hipEventRecord(ds.done[k % 2], ctx->stream));
  ds.counted = k + 1;
  return IFE_OK;
}

int dense_stream_begin(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                       const void *gen_mask, int gen_mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                       int n_sigmas, const DenseGeom &g, const float *edges, int n_edges, int block_mb,
                       int64_t *max_block_rows, int mem) {
  auto &ds = ctx->ds;
  int rc;
  const size_t nvox = (size_t)g.nvox;
  const int ncol = n_sigmas * IFE_NUM_FEATURES, nb = n_edges + 1;
  // every upload before the count of the centres comes back, which waits for them: the caller may
  // reuse its host arrays once _begin returns
  DenseInputs in;
  const void *dI;
  if ((rc = dense_stage(ctx, mem, mask, mask_dtype, gen_mask, gen_mask_dtype, nvox, edges,
                        (size_t)ncol * n_edges * 4, IFE_MEM_HOST, &in)))
    return rc;
  if ((rc = stage_in(ctx, mem, image, nvox * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  // the centres, and per centre plane the number of its first region
  DenseCentres cen;
  rc = dense_centres(ctx, in.gen, in.gen_dtype, g, ds.centres, INT64_MAX, &ds.n_rois, &cen);
  if (rc || cen.n == 0) return rc;
  const int64_t nplanes = g.nz - g.sz + 1;
  std::vector<uint32_t> first((size_t)nplanes);
  if ((rc = ensure(ctx, ctx->st_out, (size_t)nplanes * 4))) return rc;
  {
    ProfScope ps(ctx, KK_DENSE_CODE);
    hipLaunchKernelGGL(dense_plane_first_kernel, dim3((unsigned)((nplanes + 255) / 256)), dim3(256), 0, ctx->stream,
                       cen.seg_base, (uint32_t *)ctx->st_out.p, (int64_t)g.gx * g.ny, (int64_t)g.hz, nplanes);
    IFE_HIP(ctx, hipGetLastError());
  }
  IFE_HIP(ctx, hipMemcpyAsync(first.data(), ctx->st_out.p, (size_t)nplanes * 4, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<int64_t> plane_rows((size_t)nplanes);
  for (int64_t o = 0; o < nplanes; ++o)
    plane_rows[(size_t)o] = (o + 1 < nplanes ? (int64_t)first[(size_t)o + 1] : cen.n) - (int64_t)first[(size_t)o];
  // the budget: features of a group of scales (at most half, as in ife_bag_image_dense), the codes,
  // and of the rest an eighth per block buffer (three of them) and half for the box passes
  // (IFE_OPT_DIFFERENTIAL: no feature share -- the labels only, behind the jet workspace, which lies
  // outside the bound as the finite-difference workspace does)
  const bool differential = ctx->differential != 0;
  if (differential && (rc = reserve_scales(ctx, vol, true))) return rc;
  size_t budget;
  if ((rc = dense_budget(ctx, ctx->dn_feat.cap, &budget))) return rc;
  const DenseScalePlan plan =
      differential ? DenseScalePlan{0, 0, (nvox + 15) / 16 * 16} : dense_scale_plan(budget / 2, nvox, n_sigmas);
  const size_t cbytes = (size_t)ncol * nvox;
  const size_t rest = budget > plan.fbytes + cbytes ? budget - plan.fbytes - cbytes : 0;
  const size_t row_bytes = (size_t)ncol * nb * 4;
  ds.blocks = dense_plan(plane_rows, row_bytes, block_mb > 0 ? (size_t)block_mb << 20 : rest / 8, g.sz);
  int64_t max_rows = 0, max_planes = 0;
  for (const DenseBlock &b : ds.blocks) {
    max_rows = std::max(max_rows, b.n_rows);
    max_planes = std::max(max_planes, b.zc1 - b.zc0 + g.sz - 1);
  }
  const size_t bvox = (size_t)(g.nx * g.ny * max_planes);
  if ((rc = dense_groups(ctx, rest / 2, bvox, ncol, nb, 0, &ds.cg, &ds.bg))) return rc;
  ds.g = g;
  ds.flag = cen.flag;
  ds.seg_base = cen.seg_base;
  ds.ncol = ncol;
  ds.nb = nb;
  ds.ld = (max_rows + 63) / 64 * 64;
  if ((rc = ensure(ctx, ds.codes, cbytes))) return rc;
  if ((rc = ensure(ctx, ds.ws, bvox * 3 * ds.cg * ds.bg))) return rc;
  if ((rc = ensure(ctx, ds.planar, (size_t)ds.ld * row_bytes))) return rc;
  for (size_t i = 0; i < std::min<size_t>(ds.blocks.size(), 2); ++i) {
    if ((rc = ensure(ctx, ds.rows[i], (size_t)max_rows * row_bytes))) return rc;
    IFE_HIP(ctx, hipEventCreateWithFlags(&ds.done[i], hipEventDisableTiming));
  }
  if (!ds.copy) IFE_HIP(ctx, hipStreamCreateWithFlags(&ds.copy, hipStreamNonBlocking));
  auto code_scale = [&](int s, const float *feat, const uint8_t *clamp) {  // only the codes stay
    return dense_code(ctx, feat, g.nvox, 1, 0, IFE_NUM_FEATURES, clamp, IFE_U8, g.nvox,
                      in.edges + (size_t)s * IFE_NUM_FEATURES * n_edges, n_edges,
                      (uint8_t *)ds.codes.p + (size_t)s * IFE_NUM_FEATURES * nvox);
  };
  if (differential)  // the codes straight from the jet into their place
    rc = dense_code_scales(ctx, dI, image_dtype, in.mask, mask_dtype, vol, sigmas, n_sigmas, in.edges, n_edges,
                           plan.fbytes, [&](int s) { return (uint8_t *)ds.codes.p + (size_t)s * IFE_NUM_FEATURES * nvox; },
                           [](int, const uint8_t *, const uint8_t *) { return (int)IFE_OK; });
  else
    rc = dense_scale_loop(ctx, dI, image_dtype, in.mask, mask_dtype, vol, sigmas, n_sigmas, plan, code_scale);
  if (rc) return rc;
  *max_block_rows = max_rows;
  return dense_stream_count(ctx, 0);  // the first block is under way when _begin returns
}

}  // namespace

extern "C" {

int ife_bag_dense_stream_begin(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                               const void *gen_mask, int gen_mask_dtype, const ife_volume_desc *vol,
                               const float *sigmas, int n_sigmas, const int64_t size[3], const float *edges,
                               int n_edges, int values, int block_mb, int64_t *n_rois, int64_t *max_block_rows,
                               int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, true))) return rc;
  if (!image || !sigmas) return fail(ctx, IFE_E_ARG, "null pointer");
  // max_block_rows stands where the bag calls have their output array: it must not be null either
  if ((rc = dense_hist_check(ctx, mask, mask_dtype, gen_mask, gen_mask_dtype, edges, n_edges, max_block_rows, 0,
                             n_rois, mem)))
    return rc;
  if ((rc = check_sigmas(ctx, sigmas, n_sigmas))) return rc;
  if ((rc = check_image_dtype(ctx, image_dtype))) return rc;
  if (values != IFE_BAG_COUNTS && values != IFE_BAG_FREQUENCIES)
    return fail(ctx, IFE_E_ARG, "values must be IFE_BAG_COUNTS or IFE_BAG_FREQUENCIES");
  if (block_mb < 0) return fail(ctx, IFE_E_ARG, "the block bound must be >= 0 MiB");
  DenseGeom g;
  bool empty = false;
  if ((rc = dense_geom(ctx, vol, size, true, &g, &empty))) return rc;
  dense_stream_release(ctx);  // drop an earlier, unfinished stream
  *n_rois = 0;
  *max_block_rows = 0;
  ctx->ds.values = values;
  ctx->ds.open = true;  // zero regions is a stream too: its first _next reports the end
  if (empty) return IFE_OK;
  rc = dense_stream_begin(ctx, image, image_dtype, mask, mask_dtype, gen_mask, gen_mask_dtype, vol, sigmas, n_sigmas,
                          g, edges, n_edges, block_mb, max_block_rows, mem);
  if (rc) {
    dense_stream_release(ctx);
    return rc;
  }
  *n_rois = ctx->ds.n_rois;
  return IFE_OK;
}

int ife_bag_dense_stream_next(ife_ctx *ctx, void *rows, int64_t capacity_rows, int64_t *row0, int64_t *n_rows) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!row0 || !n_rows) return fail(ctx, IFE_E_ARG, "null pointer");
  auto &ds = ctx->ds;
  if (!ds.open) return fail(ctx, IFE_E_STATE, "no dense stream is open (ife_bag_dense_stream_begin starts one)");
  if (ds.next == ds.blocks.size()) {
    *row0 = ds.n_rois;
    *n_rows = 0;
    return IFE_OK;
  }
  const size_t k = ds.next;
  const DenseBlock &b = ds.blocks[k];
  *row0 = b.row0;
  *n_rows = b.n_rows;
  if (capacity_rows < b.n_rows)
    return fail(ctx, IFE_E_SIZE, "the block has %lld rows, the array holds %lld", (long long)b.n_rows,
                (long long)capacity_rows);
  if (!rows) return fail(ctx, IFE_E_ARG, "null pointer");
  if (ds.counted <= k && (rc = dense_stream_count(ctx, k))) return rc;
  // the next block is counted (into the other buffer) while this one is copied; the copy of the
  // block before it out of that buffer has finished, the _next that delivered it waited for it
  if (k + 1 < ds.blocks.size() && ds.counted <= k + 1 && (rc = dense_stream_count(ctx, k + 1))) return rc;
  IFE_HIP(ctx, hipStreamWaitEvent(ds.copy, ds.done[k % 2], 0));
  IFE_HIP(ctx, hipMemcpyAsync(rows, ds.rows[k % 2].p, (size_t)b.n_rows * ds.ncol * ds.nb * 4, hipMemcpyDeviceToHost,
                              ds.copy));
  IFE_HIP(ctx, hipStreamSynchronize(ds.copy));
  ds.next = k + 1;
  return IFE_OK;
}

int ife_bag_dense_stream_end(ife_ctx *ctx) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!ctx->ds.open) return fail(ctx, IFE_E_STATE, "no dense stream is open");
  dense_stream_release(ctx);
  return IFE_OK;
}

}  // extern "C"
