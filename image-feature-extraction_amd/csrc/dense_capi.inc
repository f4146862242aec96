// dense_capi.inc -- the dense bag entry points of include/ife_hip.h (ife_dense_rois,
// ife_dense_roi_histograms, ife_bag_image_dense); included at the end of ife_capi.hip (shares its
// context, staging and profiling helpers, and clamp01 / the scans of stats_capi.inc).

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

// Flags and numbers the centres of `gen` (device) into ctx->dn_centres; blocks for the count.
int dense_centres(ife_ctx *ctx, const void *dG, int gen_dtype, const DenseGeom &g, DenseCentres *out) {
  const int64_t nseg = (int64_t)g.gx * g.ny * g.nz;
  const int64_t nchunks = (nseg + SCAN_CHUNK - 1) / SCAN_CHUNK;
  const size_t off_flag = (8 + (size_t)(nseg + nchunks) * 4 + 15) / 16 * 16;
  int rc = ensure(ctx, ctx->dn_centres, off_flag + (size_t)g.nvox);
  if (rc) return rc;
  unsigned long long *ctr = (unsigned long long *)ctx->dn_centres.p;
  uint32_t *segs = (uint32_t *)((char *)ctx->dn_centres.p + 8), *sums = segs + nseg;
  uint8_t *flag = (uint8_t *)ctx->dn_centres.p + off_flag;
  {
    ProfScope ps(ctx, KK_DENSE_CODE);
    rc = with_mask_type(true, gen_dtype, dG, [&](auto gen) -> int {
      using TM = std::remove_cv_t<std::remove_pointer_t<decltype(gen)>>;
      hipLaunchKernelGGL(dense_centre_kernel<TM>, dim3(dense_blocks(nseg)), dim3(256), 0, ctx->stream, gen, flag,
                         segs, g, nseg);
      return IFE_OK;
    });
    hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)nchunks), dim3(SORT_THREADS), 0, ctx->stream, segs, nseg, sums);
    hipLaunchKernelGGL(scan_chunks_kernel, dim3(1), dim3(SORT_THREADS), 0, ctx->stream, sums, (int)nchunks, ctr);
    hipLaunchKernelGGL(chunk_scan_kernel, dim3((unsigned)nchunks), dim3(SORT_THREADS), 0, ctx->stream, segs, nseg, sums);
    IFE_HIP(ctx, hipGetLastError());
  }
  unsigned long long h = 0;
  IFE_HIP(ctx, hipMemcpyAsync(&h, ctr, 8, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out->flag = flag;
  out->seg_base = segs;
  out->nseg = nseg;
  out->n = (int64_t)h;
  return rc;
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

// The box counts of components [0, ncomp) of one feature volume (device), written at the centres:
// dCounts[number * row_words + col0 + c * (n_edges + 1) + bin].  dEdges: [ncomp][n_edges], device.
// Scratch per group of cg components and bg bins: nvox * cg * (1 + 3 * bg) bytes (codes; one byte
// after x and two after y per plane), sized from `budget`.
int dense_count(ife_ctx *ctx, const float *dF, int layout, int ncomp, const void *dM, int mask_dtype,
                const DenseGeom &g, const DenseCentres &cen, const float *dEdges, int n_edges, uint32_t *dCounts,
                int64_t row_words, int64_t col0, size_t budget) {
  const int nb = n_edges + 1;
  const size_t nvox = (size_t)g.nvox;
  // whole components while they fit, else one component and as many bins as fit
  int cg = (int)std::min<size_t>({(size_t)ncomp, budget / (nvox * (1 + 3 * (size_t)nb)), (size_t)1024});
  int bg = nb;
  if (cg < 1) {
    cg = 1;
    bg = budget > nvox ? (int)std::min<size_t>((budget - nvox) / (3 * nvox), (size_t)nb) : 0;
    if (bg < 1)
      return fail(ctx, IFE_E_NOMEM, "the dense box counts need %zu bytes of scratch for one bin, %zu are available",
                  4 * nvox, budget);
  }
  const size_t planes = (size_t)cg * bg;
  int rc = ensure(ctx, ctx->dn_ws, nvox * (3 * planes + cg));
  if (rc) return rc;
  uint16_t *ys = (uint16_t *)ctx->dn_ws.p;  // [planes][nvox], then xs [planes][nvox], then codes [cg][nvox]
  uint8_t *xs = (uint8_t *)(ys + planes * nvox), *code = xs + planes * nvox;
  const int64_t comp_stride = layout == IFE_PLANAR ? g.nvox : 1, vox_stride = layout == IFE_PLANAR ? 1 : ncomp;
  // marching passes: a wave covers `chunk` outputs after a start-up of (window - 1) reads
  const int64_t nyv = g.ny - g.sy + 1, nzv = g.nz - g.sz + 1;
  const int ychunk = (int)std::min<int64_t>(std::max<int64_t>(2 * (int64_t)g.sy, 64), nyv);
  const int zchunk = (int)std::min<int64_t>(std::max<int64_t>(2 * (int64_t)g.sz, 64), nzv);
  const int nych = (int)((nyv + ychunk - 1) / ychunk), nzch = (int)((nzv + zchunk - 1) / zchunk);
  for (int c0 = 0; c0 < ncomp; c0 += cg) {
    const int nc = std::min(cg, ncomp - c0);
    {
      ProfScope ps(ctx, KK_DENSE_CODE);
      const dim3 grid((unsigned)std::min<int64_t>((g.nvox + 255) / 256, 1 << 16), (unsigned)nc);
      rc = with_mask_type(true, mask_dtype, dM, [&](auto msk) -> int {
        using TM = std::remove_cv_t<std::remove_pointer_t<decltype(msk)>>;
        hipLaunchKernelGGL(dense_code_kernel<TM>, grid, dim3(256), 0, ctx->stream, dF, msk, dEdges, code, g.nvox,
                           comp_stride, vox_stride, c0, n_edges);
        IFE_HIP(ctx, hipGetLastError());
        return IFE_OK;
      });
      if (rc) return rc;
    }
    for (int b0 = 0; b0 < nb; b0 += bg) {
      const int nbins = std::min(bg, nb - b0);
      const int64_t np = (int64_t)nc * nbins;
      {
        ProfScope ps(ctx, KK_DENSE_XY);
        const int64_t wx = (int64_t)g.gx * g.ny * g.nz * nc, wy = (int64_t)g.gx * g.nz * nych * np;
        hipLaunchKernelGGL(dense_box_x_kernel, dim3(dense_blocks(wx)), dim3(256), 0, ctx->stream, code, xs, g, b0,
                           nbins, wx);
        hipLaunchKernelGGL(dense_box_y_kernel, dim3(dense_blocks(wy)), dim3(256), 0, ctx->stream, xs, ys, g, ychunk,
                           nych, wy);
      }
      {
        ProfScope ps(ctx, KK_DENSE_Z);
        const int64_t wz = (int64_t)g.gx * nyv * nzch * np;
        hipLaunchKernelGGL(dense_box_z_kernel, dim3(dense_blocks(wz)), dim3(256), 0, ctx->stream, ys, cen.flag,
                           cen.seg_base, dCounts, g, nbins, nb, row_words, col0 + (int64_t)c0 * nb + b0, zchunk, nzch,
                           wz);
      }
      IFE_HIP(ctx, hipGetLastError());
    }
  }
  return IFE_OK;
}

// Arguments shared by the two histogram calls (everything but their inputs).
int dense_hist_check(ife_ctx *ctx, const void *mask, int mask_dtype, const void *gen_mask, int gen_mask_dtype,
                     const float *edges, int n_edges, const uint32_t *counts, int64_t capacity,
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

int dense_too_many(ife_ctx *ctx, int64_t n, int64_t capacity) {
  return fail(ctx, IFE_E_SIZE, "%lld regions, the output holds %lld", (long long)n, (long long)capacity);
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
  DenseCentres cen;
  if ((rc = dense_centres(ctx, dG, gen_mask_dtype, g, &cen))) return rc;
  *n_rois = cen.n;
  if (!rois || cen.n == 0) return IFE_OK;
  if (cen.n > capacity) return dense_too_many(ctx, cen.n, capacity);
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
  const size_t nvox = (size_t)g.nvox, gbytes = gen_mask ? nvox * dtype_size(gen_mask_dtype) : 0;
  const size_t ebytes = (size_t)ncomp * n_edges * 4, off_e = (gbytes + 15) / 16 * 16;
  const void *dM, *dG = nullptr, *dE = edges, *dF;
  if ((rc = stage_in(ctx, mem, mask, nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
  if (mem == IFE_MEM_HOST) {  // the generating mask and the edges share one staging buffer
    if ((rc = ensure(ctx, ctx->st_aux, off_e + ebytes))) return rc;
    if (gen_mask) IFE_HIP(ctx, hipMemcpyAsync(ctx->st_aux.p, gen_mask, gbytes, hipMemcpyHostToDevice, ctx->stream));
    IFE_HIP(ctx, hipMemcpyAsync((char *)ctx->st_aux.p + off_e, edges, ebytes, hipMemcpyHostToDevice, ctx->stream));
    dG = gen_mask ? ctx->st_aux.p : nullptr;
    dE = (char *)ctx->st_aux.p + off_e;
  } else {
    dG = gen_mask;
  }
  DenseCentres cen;
  if ((rc = dense_centres(ctx, dG ? dG : dM, dG ? gen_mask_dtype : mask_dtype, g, &cen))) return rc;
  *n_rois = cen.n;
  if (cen.n > capacity) return dense_too_many(ctx, cen.n, capacity);
  if (cen.n == 0) return IFE_OK;
  if ((rc = stage_in(ctx, mem, features, nvox * ncomp * 4, ctx->st_img, &dF))) return rc;
  const size_t cbytes = (size_t)cen.n * ncomp * (n_edges + 1) * 4;
  void *dC;
  if ((rc = stage_out_begin(ctx, mem, counts, cbytes, &dC))) return rc;
  size_t budget;
  if ((rc = dense_budget(ctx, ctx->dn_ws.cap, &budget))) return rc;
  if ((rc = dense_count(ctx, (const float *)dF, layout, ncomp, dM, mask_dtype, g, cen, (const float *)dE, n_edges,
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
  const size_t nvox = (size_t)g.nvox, gbytes = gen_mask ? nvox * dtype_size(gen_mask_dtype) : 0;
  const int ncol = n_sigmas * IFE_NUM_FEATURES, nb = n_edges + 1;
  const size_t ebytes = (size_t)ncol * n_edges * 4, off_e = (gbytes + 15) / 16 * 16;
  const void *dI, *dM, *dG = gen_mask;
  if ((rc = stage_in(ctx, mem, mask, nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
  if ((rc = ensure(ctx, ctx->st_aux, off_e + ebytes))) return rc;  // generating mask (HOST mode), edges
  if (gen_mask && mem == IFE_MEM_HOST) {
    IFE_HIP(ctx, hipMemcpyAsync(ctx->st_aux.p, gen_mask, gbytes, hipMemcpyHostToDevice, ctx->stream));
    dG = ctx->st_aux.p;
  }
  const float *dE = (const float *)((char *)ctx->st_aux.p + off_e);
  IFE_HIP(ctx, hipMemcpyAsync((char *)ctx->st_aux.p + off_e, edges, ebytes, hipMemcpyHostToDevice, ctx->stream));
  DenseCentres cen;
  if ((rc = dense_centres(ctx, dG ? dG : dM, dG ? gen_mask_dtype : mask_dtype, g, &cen))) return rc;
  *n_rois = cen.n;
  if (cen.n > capacity) return dense_too_many(ctx, cen.n, capacity);
  if (cen.n == 0) return IFE_OK;
  if ((rc = stage_in(ctx, mem, image, nvox * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  const size_t cbytes = (size_t)cen.n * ncol * nb * 4;
  if ((rc = ensure(ctx, ctx->st_out, cbytes))) return rc;
  // scales in groups: the clamped labels and the features of `sg` scales (32 bytes per voxel and
  // scale) take at most half of the budget, the box counts get the rest
  size_t budget;
  if ((rc = dense_budget(ctx, ctx->dn_ws.cap + ctx->dn_feat.cap, &budget))) return rc;
  const size_t scale_bytes = nvox * IFE_NUM_FEATURES * 4, off_f = (nvox + 15) / 16 * 16;
  const int sg = (int)std::min<size_t>(std::max<size_t>(budget / 2 / scale_bytes, 1), (size_t)n_sigmas);
  const size_t fbytes = off_f + (size_t)sg * scale_bytes;
  if ((rc = ensure(ctx, ctx->dn_feat, fbytes))) return rc;
  uint8_t *clamp = (uint8_t *)ctx->dn_feat.p;
  float *feat = (float *)((char *)ctx->dn_feat.p + off_f);
  if ((rc = launch_clamp01(ctx, dM, mask_dtype, clamp, g.nvox))) return rc;
  for (int s0 = 0; s0 < n_sigmas; s0 += sg) {
    const int ns = std::min(sg, n_sigmas - s0);
    if ((rc = ife_emphysema_features(ctx, dI, image_dtype, clamp, IFE_U8, vol, sigmas + s0, ns, feat, IFE_PLANAR,
                                     IFE_MEM_DEVICE)))
      return rc;
    for (int i = 0; i < ns; ++i)
      if ((rc = dense_count(ctx, feat + (size_t)i * nvox * IFE_NUM_FEATURES, IFE_PLANAR, IFE_NUM_FEATURES, clamp,
                            IFE_U8, g, cen, dE + (size_t)(s0 + i) * IFE_NUM_FEATURES * n_edges, n_edges,
                            (uint32_t *)ctx->st_out.p, (int64_t)ncol * nb, (int64_t)(s0 + i) * IFE_NUM_FEATURES * nb,
                            budget > fbytes ? budget - fbytes : 0)))
        return rc;
  }
  IFE_HIP(ctx, hipMemcpyAsync(counts, ctx->st_out.p, cbytes, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return IFE_OK;
}

}  // extern "C"
