// sampling_capi.inc -- ife_sample_positions, ife_random_rois and ife_extract_rois of
// include/ife_hip.h (DESIGN.md "Sampling"); included at the end of ife_capi.hip behind
// dense_capi.inc (dense_geom, dense_blocks) and region_capi.inc (region_volume_bytes).  The checks
// that need no device and the generator are sampling_plan.hpp's, plain host code.

namespace {

// Both sampling calls: the admissible voxels of every set counted and numbered, the counts to the
// host, then one wave per draw.  out: [sets][n_draws] positions or [sets][n_draws][6] boxes.
int sampling_draw(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol, const int *values,
                  int n_values, int per_value, const int64_t *size, uint64_t seed, uint32_t stream,
                  uint64_t first_draw, int64_t n_draws, int64_t *out, bool boxes, int64_t *n_admissible, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, false))) return rc;
  if (!n_admissible) return fail(ctx, IFE_E_ARG, "null pointer");
  SamplingSets sets;
  int64_t box[3];
  const char *msg = "";
  if ((rc = sampling_check(mask_dtype == IFE_U8 ? 255 : 65535, values, n_values, per_value, size, n_draws, &sets, box,
                           &msg)))
    return fail(ctx, rc == SAMPLING_E_SIZE ? IFE_E_SIZE : IFE_E_ARG, "%s", msg);
  if (n_draws > 0 && !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if (mem == IFE_MEM_DEVICE &&
      (reinterpret_cast<uintptr_t>(mask) % dtype_size(mask_dtype) || reinterpret_cast<uintptr_t>(out) % 8))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  DenseGeom g;
  bool empty = false;
  if ((rc = dense_geom(ctx, vol, box, false, &g, &empty))) return rc;
  for (int j = 0; j < sets.n_sets; ++j) n_admissible[j] = 0;
  const void *dM = nullptr;
  const int64_t nseg = empty ? 0 : (int64_t)g.gx * g.ny * g.nz;
  const size_t area = seg_scan_bytes(nseg);  // per set: [total][counts -> bases][chunk sums]
  if (!empty) {  // a box larger than the volume fits nowhere
    if ((rc = stage_in(ctx, mem, mask, (size_t)g.nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
    if ((rc = ensure(ctx, ctx->dn_centres, area * (size_t)sets.n_sets))) return rc;
    char *base = (char *)ctx->dn_centres.p;
    {
      ProfScope ps(ctx, KK_DENSE_CODE);
      with_mask_type(true, mask_dtype, dM, [&](auto m) -> int {
        using TM = std::remove_cv_t<std::remove_pointer_t<decltype(m)>>;
        // 4 waves of SAMPLING_COUNT_RUN consecutive segments per workgroup, longer runs beyond the cap
        const unsigned blocks = (unsigned)std::min<int64_t>(
            std::max<int64_t>((nseg + 4 * SAMPLING_COUNT_RUN - 1) / (4 * SAMPLING_COUNT_RUN), 1), 1 << 18);
        hipLaunchKernelGGL(sampling_count_kernel<TM>, dim3(blocks), dim3(256), 0, ctx->stream, m,
                           (uint32_t *)(base + 8), (int64_t)(area / 4), g, nseg, sets);
        return IFE_OK;
      });
      const int64_t nchunks = seg_scan_chunks(nseg);
      for (int j = 0; j < sets.n_sets; ++j) {
        uint32_t *segs = (uint32_t *)(base + (size_t)j * area + 8), *sums = segs + nseg;
        hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)nchunks), dim3(SORT_THREADS), 0, ctx->stream, segs, nseg,
                           sums);
        hipLaunchKernelGGL(scan_chunks_kernel, dim3(1), dim3(SORT_THREADS), 0, ctx->stream, sums, (int)nchunks,
                           (unsigned long long *)(base + (size_t)j * area));
        hipLaunchKernelGGL(chunk_scan_kernel, dim3((unsigned)nchunks), dim3(SORT_THREADS), 0, ctx->stream, segs, nseg,
                           sums);
      }
      IFE_HIP(ctx, hipGetLastError());
    }
    unsigned long long totals[SAMPLING_MAX_VALUES];
    for (int j = 0; j < sets.n_sets; ++j)
      IFE_HIP(ctx, hipMemcpyAsync(&totals[j], base + (size_t)j * area, 8, hipMemcpyDeviceToHost, ctx->stream));
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < sets.n_sets; ++j) n_admissible[j] = (int64_t)totals[j];
  }
  if (n_draws == 0) return IFE_OK;
  for (int j = 0; j < sets.n_sets; ++j)
    if (n_admissible[j] == 0) {  // the reference would draw forever
      if (sets.n_values == 0)
        return fail(ctx, IFE_E_ARG, "set 0 (mask != 0) has no voxel that admits a box of %lld x %lld x %lld",
                    (long long)box[0], (long long)box[1], (long long)box[2]);
      if (!sets.per_value)
        return fail(ctx, IFE_E_ARG, "set 0 (the %d values) has no voxel that admits a box of %lld x %lld x %lld",
                    sets.n_values, (long long)box[0], (long long)box[1], (long long)box[2]);
      return fail(ctx, IFE_E_ARG, "set %d (mask == %u) has no voxel that admits a box of %lld x %lld x %lld", j,
                  sets.values[j], (long long)box[0], (long long)box[1], (long long)box[2]);
    }
  const size_t out_bytes = (size_t)sets.n_sets * (size_t)n_draws * (boxes ? 48 : 8);
  void *dO;
  if ((rc = stage_out_begin(ctx, mem, out, out_bytes, &dO))) return rc;
  {
    ProfScope ps(ctx, KK_GATHER);
    const SamplingDraws d = {seed, first_draw, stream, n_draws, boxes ? 1 : 0};
    const int64_t waves = (int64_t)sets.n_sets * n_draws;
    const unsigned blocks = (unsigned)std::min<int64_t>((waves + 3) / 4, SAMPLING_SELECT_GRID_CAP);
    with_mask_type(true, mask_dtype, dM, [&](auto m) -> int {
      using TM = std::remove_cv_t<std::remove_pointer_t<decltype(m)>>;
      hipLaunchKernelGGL(sampling_select_kernel<TM>, dim3(blocks), dim3(256), 0, ctx->stream, m,
                         (const uint32_t *)((char *)ctx->dn_centres.p + 8), (int64_t)(area / 4), g, nseg, sets, d,
                         (int64_t *)dO);
      return IFE_OK;
    });
    IFE_HIP(ctx, hipGetLastError());
  }
  if (mem == IFE_MEM_DEVICE) {  // the call blocks in both modes
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IFE_OK;
  }
  return stage_out_end(ctx, mem, out, out_bytes);
}

template <int ES>
void launch_sampling_gather(ife_ctx *ctx, const void *dS, const int64_t *dR, int64_t n_rois, const int64_t size[3],
                            const ife_volume_desc *vol, void *dD) {
  const int64_t nrows = n_rois * size[1] * size[2];
  const unsigned blocks =
      (unsigned)std::min<int64_t>((nrows + REGION_WAVES - 1) / REGION_WAVES, SAMPLING_GATHER_GRID_CAP);
  hipLaunchKernelGGL(sampling_gather_kernel<ES>, dim3(blocks), dim3(REGION_BLOCK), 0, ctx->stream,
                     (const unsigned char *)dS, dR, nrows, size[0], size[1], size[2], vol->nx, vol->ny,
                     (unsigned char *)dD);
}

}  // namespace

extern "C" {

// ---- draws of admissible voxels: their linear indices -------------------------------------------------
int ife_sample_positions(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol,
                         const int *values, int n_values, int per_value, const int64_t *size, uint64_t seed,
                         uint32_t stream, uint64_t first_draw, int64_t n_draws, int64_t *positions,
                         int64_t *n_admissible, int mem) {
  return sampling_draw(ctx, mask, mask_dtype, vol, values, n_values, per_value, size, seed, stream, first_draw,
                       n_draws, positions, false, n_admissible, mem);
}

// ---- RegionOfInterestGenerator<TMask>::generate: the boxes around such draws ---------------------------
int ife_random_rois(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol, const int *values,
                    int n_values, int per_value, const int64_t *size, uint64_t seed, uint32_t stream,
                    uint64_t first_draw, int64_t n_draws, int64_t *rois, int64_t *n_admissible, int mem) {
  return sampling_draw(ctx, mask, mask_dtype, vol, values, n_values, per_value, size, seed, stream, first_draw,
                       n_draws, rois, true, n_admissible, mem);
}

// ---- tools/SampleROIs.cxx:151-167: RegionOfInterestImageFilter over a list of boxes of one size ---------
int ife_extract_rois(ife_ctx *ctx, const void *src, int elem_bytes, const ife_volume_desc *vol, const int64_t *rois,
                     int64_t n_rois, void *dst, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
    return fail(ctx, IFE_E_ARG, "elem_bytes must be 1, 2, 4 or 8");
  if (n_rois < 0) return fail(ctx, IFE_E_ARG, "negative count");
  if (n_rois == 0) return IFE_OK;
  if (!src || !rois || !dst) return fail(ctx, IFE_E_ARG, "null pointer");
  if (mem == IFE_MEM_DEVICE && (reinterpret_cast<uintptr_t>(src) % elem_bytes ||
                                reinterpret_cast<uintptr_t>(dst) % elem_bytes || reinterpret_cast<uintptr_t>(rois) % 8))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  const int64_t src_bytes = region_volume_bytes(vol, elem_bytes);
  if (src_bytes < 0) return fail(ctx, IFE_E_SIZE, "the source's byte count overflows");
  const int64_t n[3] = {vol->nx, vol->ny, vol->nz};
  int64_t first[6];  // the size every box must have
  if (mem == IFE_MEM_DEVICE) {
    IFE_HIP(ctx, hipMemcpyAsync(first, rois, sizeof first, hipMemcpyDeviceToHost, ctx->stream));
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  } else {
    std::memcpy(first, rois, sizeof first);
  }
  const int64_t bad = sampling_first_bad_box(mem == IFE_MEM_DEVICE ? first : rois, mem == IFE_MEM_DEVICE ? 1 : n_rois, n);
  if (bad >= 0) {
    const int64_t *q = mem == IFE_MEM_DEVICE ? first : rois + 6 * bad;
    return fail(ctx, IFE_E_ARG,
                "region %lld [%lld, %lld, %lld][%lld, %lld, %lld] is outside of the largest possible region "
                "[%lld, %lld, %lld], has a size below 1 or not the size of the first region", (long long)bad,
                (long long)q[0], (long long)q[1], (long long)q[2], (long long)q[3], (long long)q[4], (long long)q[5],
                (long long)n[0], (long long)n[1], (long long)n[2]);
  }
  const int64_t dst_bytes = sampling_gather_bytes(n_rois, first + 3, elem_bytes);
  if (dst_bytes < 0) return fail(ctx, IFE_E_SIZE, "the regions hold more than 2^40 bytes");
  if (mem == IFE_MEM_DEVICE && region_ranges_overlap(src, (size_t)src_bytes, dst, (size_t)dst_bytes))
    return fail(ctx, IFE_E_ARG, "src and dst overlap");
  const void *dS, *dR;
  if ((rc = stage_in(ctx, mem, src, (size_t)src_bytes, ctx->st_img, &dS))) return rc;
  if ((rc = stage_in(ctx, mem, rois, (size_t)n_rois * 48, ctx->st_aux, &dR))) return rc;
  if (mem == IFE_MEM_DEVICE) {  // the boxes are checked where they are, before anything reads through them
    if ((rc = ensure(ctx, ctx->st_mask, 16))) return rc;
    int flag = 0;
    IFE_HIP(ctx, hipMemsetAsync(ctx->st_mask.p, 0, 4, ctx->stream));
    {
      ProfScope ps(ctx, KK_GATHER);
      hipLaunchKernelGGL(sampling_box_check_kernel, dim3((unsigned)std::min<int64_t>((n_rois + 255) / 256, 2048)),
                         dim3(256), 0, ctx->stream, (const int64_t *)dR, n_rois, first[3], first[4], first[5], n[0],
                         n[1], n[2], (int *)ctx->st_mask.p);
      IFE_HIP(ctx, hipGetLastError());
    }
    IFE_HIP(ctx, hipMemcpyAsync(&flag, ctx->st_mask.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (flag)
      return fail(ctx, IFE_E_ARG, "a region is outside of the largest possible region [%lld, %lld, %lld] or has not "
                  "the size of the first region", (long long)n[0], (long long)n[1], (long long)n[2]);
  }
  void *dD;
  if ((rc = stage_out_begin(ctx, mem, dst, (size_t)dst_bytes, &dD))) return rc;
  {
    ProfScope ps(ctx, KK_GATHER);
    switch (elem_bytes) {
      case 1: launch_sampling_gather<1>(ctx, dS, (const int64_t *)dR, n_rois, first + 3, vol, dD); break;
      case 2: launch_sampling_gather<2>(ctx, dS, (const int64_t *)dR, n_rois, first + 3, vol, dD); break;
      case 4: launch_sampling_gather<4>(ctx, dS, (const int64_t *)dR, n_rois, first + 3, vol, dD); break;
      default: launch_sampling_gather<8>(ctx, dS, (const int64_t *)dR, n_rois, first + 3, vol, dD); break;
    }
    IFE_HIP(ctx, hipGetLastError());
  }
  if (mem == IFE_MEM_DEVICE) {  // the call blocks in both modes
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IFE_OK;
  }
  return stage_out_end(ctx, mem, dst, (size_t)dst_bytes);
}

}  // extern "C"
