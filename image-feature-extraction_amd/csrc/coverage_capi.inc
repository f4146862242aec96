// coverage_capi.inc -- ife_value_census_f32, ife_threshold_mask and ife_roi_coverage of
// include/ife_hip.h (DESIGN.md "Census and coverage"); included at the end of ife_capi.hip behind
// stats_capi.inc (sort_columns, seg_scan, scan_total), region_capi.inc (region_ranges_overlap) and
// sampling_capi.inc.  The checks that need no device are coverage_plan.hpp's, plain host code.

namespace {

int coverage_fail(ife_ctx *ctx, int rc, const char *msg) {
  return fail(ctx, rc == COVERAGE_E_SIZE ? IFE_E_SIZE : IFE_E_ARG, "%s", msg);
}

uint32_t float_bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

}  // namespace

extern "C" {

// ---- tools/ImageBrowser.cxx:165-173: std::set<float> and a DenseHistogram over its values ---------------
int ife_value_census_f32(ife_ctx *ctx, const float *values, int64_t n, float *uniq, uint32_t *counts,
                         int64_t capacity, int64_t *n_unique, int64_t *n_nan, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  const char *msg = "";
  if ((rc = census_check(values != nullptr, n, uniq != nullptr, counts != nullptr, capacity, n_unique != nullptr,
                         n_nan != nullptr, &msg)))
    return coverage_fail(ctx, rc, msg);
  if (mem == IFE_MEM_DEVICE && (reinterpret_cast<uintptr_t>(values) % 4 || reinterpret_cast<uintptr_t>(uniq) % 4 ||
                                reinterpret_cast<uintptr_t>(counts) % 4))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  // the sorted copy, the sort's partner (the head positions afterwards) and the segment counts with
  // the two NaN counters behind them
  const int64_t nseg = (n + CENSUS_SEG - 1) / CENSUS_SEG;
  const size_t scan_bytes = seg_scan_bytes(nseg);
  if ((rc = ensure(ctx, ctx->dn_ws, (size_t)n * 4))) return rc;
  if ((rc = ensure(ctx, ctx->st_aux, (size_t)n * 4))) return rc;
  if ((rc = ensure(ctx, ctx->dn_centres, scan_bytes + 16))) return rc;
  uint32_t *sorted = (uint32_t *)ctx->dn_ws.p, *positions = (uint32_t *)ctx->st_aux.p;
  unsigned long long *nans = (unsigned long long *)((char *)ctx->dn_centres.p + scan_bytes);
  IFE_HIP(ctx, hipMemcpyAsync(sorted, values, (size_t)n * 4,
                              mem == IFE_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = sort_columns(ctx, (float *)sorted, (float *)positions, ctx->st_img, ctx->st_mask, 1, n, n))) return rc;
  IFE_HIP(ctx, hipMemsetAsync(nans, 0, 16, ctx->stream));
  const unsigned seg_blocks = (unsigned)std::min<int64_t>((nseg + 3) / 4, CENSUS_GRID_CAP);
  {
    ProfScope ps(ctx, KK_SORT_SCAN);
    hipLaunchKernelGGL(census_heads_kernel, dim3(seg_blocks), dim3(256), 0, ctx->stream, sorted, n, nseg,
                       seg_counts(ctx->dn_centres), nans);
    if ((rc = seg_scan(ctx, ctx->dn_centres, nseg))) return rc;
  }
  int64_t runs = 0;
  unsigned long long h_nans[2] = {0, 0};
  IFE_HIP(ctx, hipMemcpyAsync(h_nans, nans, 16, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = scan_total(ctx, ctx->dn_centres, &runs))) return rc;  // blocks
  *n_unique = runs;
  *n_nan = (int64_t)(h_nans[0] + h_nans[1]);
  if (runs > capacity) {
    if (capacity == 0 && !uniq) return IFE_OK;  // the counts alone
    return fail(ctx, IFE_E_ARG, "the array holds %lld distinct values, the outputs have room for %lld",
                (long long)runs, (long long)capacity);
  }
  if (runs == 0) return IFE_OK;
  // HOST mode: both outputs in one staging area, the counts behind the values
  const size_t out_bytes = (size_t)runs * 4;
  void *dU = uniq, *dC = counts;
  if (mem == IFE_MEM_HOST) {
    if ((rc = stage_out_begin(ctx, mem, uniq, 2 * out_bytes, &dU))) return rc;
    dC = (char *)dU + out_bytes;
  }
  {
    ProfScope ps(ctx, KK_GATHER);
    hipLaunchKernelGGL(census_positions_kernel, dim3(seg_blocks), dim3(256), 0, ctx->stream, sorted, n, nseg,
                       seg_counts(ctx->dn_centres), positions);
    hipLaunchKernelGGL(census_runs_kernel, dim3((unsigned)std::min<int64_t>((runs + 255) / 256, CENSUS_GRID_CAP)),
                       dim3(256), 0, ctx->stream, sorted, positions, runs, (uint32_t)(n - (int64_t)h_nans[1]),
                       (uint32_t *)dU, (uint32_t *)dC);
    IFE_HIP(ctx, hipGetLastError());
  }
  if (mem == IFE_MEM_HOST) {
    IFE_HIP(ctx, hipMemcpyAsync(uniq, dU, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    IFE_HIP(ctx, hipMemcpyAsync(counts, dC, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the call blocks in both modes
  return IFE_OK;
}

// ---- itk::BinaryThresholdImageFilter as tools/ImageBrowser.cxx:35-42 sets it ----------------------------
int ife_threshold_mask(ife_ctx *ctx, const float *image, int64_t n, float low, float high, uint8_t *mask,
                       int64_t *count, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  const uint32_t lo = float_bits(low), hi = float_bits(high);
  const char *msg = "";
  if ((rc = threshold_check(image != nullptr, mask != nullptr, n, lo, hi, &msg))) return coverage_fail(ctx, rc, msg);
  if (mem == IFE_MEM_DEVICE) {
    if (reinterpret_cast<uintptr_t>(image) % 4)
      return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
    if (region_ranges_overlap(image, (size_t)n * 4, mask, (size_t)n)) return fail(ctx, IFE_E_ARG, "image and mask overlap");
  }
  const void *dI;
  void *dM;
  if ((rc = stage_in(ctx, mem, image, (size_t)n * 4, ctx->st_img, &dI))) return rc;
  if ((rc = stage_out_begin(ctx, mem, mask, (size_t)n, &dM))) return rc;
  if ((rc = ensure(ctx, ctx->st_aux, 16))) return rc;
  unsigned long long *dCount = (unsigned long long *)ctx->st_aux.p;
  IFE_HIP(ctx, hipMemsetAsync(dCount, 0, 8, ctx->stream));
  {
    ProfScope ps(ctx, KK_MASK);
    const int64_t head = std::min<int64_t>(n, (int64_t)((0 - reinterpret_cast<uintptr_t>(dI)) & 15u) / 4);
    const bool packed = (reinterpret_cast<uintptr_t>(dM) + (uintptr_t)head) % 4 == 0;
    const int64_t pieces = (n - head) / 4;
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((pieces + 255) / 256, 1), THRESHOLD_GRID_CAP);
    hipLaunchKernelGGL(threshold_mask_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const uint32_t *)dI, n, head,
                       coverage_order_image(lo), coverage_order_image(hi), packed, (uint8_t *)dM, dCount);
    IFE_HIP(ctx, hipGetLastError());
  }
  unsigned long long ones = 0;
  IFE_HIP(ctx, hipMemcpyAsync(&ones, dCount, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (mem == IFE_MEM_HOST) {
    if ((rc = stage_out_end(ctx, mem, mask, (size_t)n))) return rc;
  } else {
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the call blocks in both modes
  }
  if (count) *count = (int64_t)ones;
  return IFE_OK;
}

// ---- tools/ImageBrowser.cxx:59-99: the visited volume of a growing list of boxes, counted per round -------
int ife_roi_coverage(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol, const int64_t *rois,
                     int64_t n_rois, const int64_t *round_ends, int n_rounds, int64_t *visited, int64_t *hits,
                     int64_t *region_size, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, false))) return rc;
  const char *msg = "";
  if ((rc = coverage_check_rounds(round_ends, n_rounds, n_rois, &msg))) return coverage_fail(ctx, rc, msg);
  if (!visited || !hits || (n_rois > 0 && !rois)) return fail(ctx, IFE_E_ARG, "null pointer");
  if (mem == IFE_MEM_DEVICE &&
      (reinterpret_cast<uintptr_t>(mask) % dtype_size(mask_dtype) || reinterpret_cast<uintptr_t>(rois) % 8))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  const int64_t nvox = coverage_voxels(vol->nx, vol->ny, vol->nz);
  if (nvox < 0) return fail(ctx, IFE_E_SIZE, "the volume holds more than 2^32-1 voxels");
  if (n_rois > SAMPLING_MAX_OUTPUTS) return fail(ctx, IFE_E_SIZE, "more than 2^36 boxes");
  const int64_t n[3] = {vol->nx, vol->ny, vol->nz};
  if (mem == IFE_MEM_HOST) {
    const int64_t bad = coverage_first_bad_box(rois, n_rois, n);
    if (bad >= 0) {
      const int64_t *q = rois + 6 * bad;
      return fail(ctx, IFE_E_ARG,
                  "region %lld [%lld, %lld, %lld][%lld, %lld, %lld] is outside of the largest possible region "
                  "[%lld, %lld, %lld] or has a size below 1", (long long)bad, (long long)q[0], (long long)q[1],
                  (long long)q[2], (long long)q[3], (long long)q[4], (long long)q[5], (long long)n[0],
                  (long long)n[1], (long long)n[2]);
    }
  }
  const void *dM, *dR;
  if ((rc = stage_in(ctx, mem, mask, (size_t)nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
  if ((rc = stage_in(ctx, mem, n_rois ? rois : nullptr, (size_t)n_rois * 48, ctx->st_aux, &dR))) return rc;
  // the two planes, each padded to whole groups of the plane kernel, and the counters
  const int64_t nwords = coverage_words(nvox);
  const int64_t ngroups = (nvox + COVERAGE_GROUP - 1) / COVERAGE_GROUP, plane_words = ngroups * (COVERAGE_GROUP / 32);
  if ((rc = ensure(ctx, ctx->dn_ws, (size_t)plane_words * 8))) return rc;
  if ((rc = ensure(ctx, ctx->dn_centres, sizeof(CoverageCounters)))) return rc;
  uint32_t *dV = (uint32_t *)ctx->dn_ws.p, *dP = dV + plane_words;
  CoverageCounters *dC = (CoverageCounters *)ctx->dn_centres.p;
  IFE_HIP(ctx, hipMemsetAsync(dC, 0, sizeof(CoverageCounters), ctx->stream));
  if (mem == IFE_MEM_DEVICE && n_rois > 0) {  // the boxes are checked where they are, before anything is painted
    int flag = 0;
    {
      ProfScope ps(ctx, KK_GATHER);
      hipLaunchKernelGGL(coverage_box_check_kernel, dim3((unsigned)std::min<int64_t>((n_rois + 255) / 256, 2048)),
                         dim3(256), 0, ctx->stream, (const int64_t *)dR, n_rois, n[0], n[1], n[2], dC);
      IFE_HIP(ctx, hipGetLastError());
    }
    IFE_HIP(ctx, hipMemcpyAsync(&flag, &dC->bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (flag)
      return fail(ctx, IFE_E_ARG, "a region is outside of the largest possible region [%lld, %lld, %lld] or has a "
                  "size below 1", (long long)n[0], (long long)n[1], (long long)n[2]);
  }
  IFE_HIP(ctx, hipMemsetAsync(dV, 0, (size_t)plane_words * 4, ctx->stream));
  {
    ProfScope ps(ctx, KK_MASK);
    const unsigned blocks = (unsigned)std::min<int64_t>((ngroups + 3) / 4, COVERAGE_PLANE_GRID_CAP);
    with_mask_type(true, mask_dtype, dM, [&](auto m) -> int {
      using TM = std::remove_cv_t<std::remove_pointer_t<decltype(m)>>;
      hipLaunchKernelGGL(coverage_plane_kernel<TM>, dim3(blocks), dim3(256), 0, ctx->stream, m, nvox, dP, dC);
      return IFE_OK;
    });
    IFE_HIP(ctx, hipGetLastError());
  }
  int64_t done = 0;  // boxes painted so far
  for (int r = 0; r < n_rounds; ++r) {
    if (round_ends[r] == done) continue;  // nothing new: the round repeats its predecessor (or is empty)
    {
      ProfScope ps(ctx, KK_GATHER);
      const unsigned blocks = (unsigned)std::min<int64_t>((round_ends[r] - done + 3) / 4, COVERAGE_PAINT_GRID_CAP);
      hipLaunchKernelGGL(coverage_paint_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const int64_t *)dR, done,
                         round_ends[r], n[0], n[1], dV);
    }
    {
      ProfScope ps(ctx, KK_HIST);
      const unsigned blocks = (unsigned)std::min<int64_t>((nwords + 255) / 256, COVERAGE_COUNT_GRID_CAP);
      hipLaunchKernelGGL(coverage_count_kernel, dim3(blocks), dim3(256), 0, ctx->stream, dV, dP, nwords,
                         coverage_tail_mask(nvox), r, dC);
    }
    IFE_HIP(ctx, hipGetLastError());
    done = round_ends[r];
  }
  CoverageCounters h;
  IFE_HIP(ctx, hipMemcpyAsync(&h, dC, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  done = 0;
  for (int r = 0; r < n_rounds; ++r) {
    const bool fresh = round_ends[r] != done;
    visited[r] = fresh ? (int64_t)h.visited[r] : r ? visited[r - 1] : 0;
    hits[r] = fresh ? (int64_t)h.hits[r] : r ? hits[r - 1] : 0;
    done = round_ends[r];
  }
  if (region_size) *region_size = (int64_t)h.region;
  return IFE_OK;
}

}  // extern "C"
