// stats_capi.inc -- row f1/f2 entry points of include/ife_hip.h; included at the end of
// ife_capi.hip (shares its context, staging and profiling helpers).

struct ife_samples {
  ife_ctx *ctx = nullptr;
  int ncol = 0;
  int64_t cap = 0;              // elements per column
  std::vector<int64_t> count;   // samples per column
  bool sorted = false;
  DevBuf data, tmp;             // [ncol][cap] float, ping-pong partner
  DevBuf table, totals;         // radix pass tables: tile offsets, segment sums
  DevBuf feat, clamp, idx;      // per-image scratch of ife_samples_add_image
  DevBuf counter, edges, status;
};

namespace {

int sort_tables(ife_ctx *ctx, DevBuf &table, DevBuf &segsum, int ncol, int64_t n) {
  const int64_t ntiles = (n + SORT_TILE - 1) / SORT_TILE;
  int rc = ensure(ctx, table, (size_t)ncol * 256 * (size_t)std::max<int64_t>(ntiles, 1) * 4);
  if (rc) return rc;
  return ensure(ctx, segsum, (size_t)ncol * SORT_SEGS * 256 * 4);
}

// LSD radix sort of ncol columns of n floats each, `stride` elements apart, in place in
// `data` (four passes: data -> tmp -> data -> tmp -> data)
int sort_columns(ife_ctx *ctx, float *data, float *tmp, DevBuf &table, DevBuf &segsum, int ncol,
                 int64_t n, int64_t stride) {
  if (n <= 1 || ncol <= 0) return IFE_OK;
  if (n >= (int64_t)1 << 31) return fail(ctx, IFE_E_SIZE, "a sample column holds at most 2^31-1 values");
  int rc = sort_tables(ctx, table, segsum, ncol, n);
  if (rc) return rc;
  SortGeom g;
  g.n = n;
  g.stride = stride;
  g.ntiles = (int)((n + SORT_TILE - 1) / SORT_TILE);
  g.seg_tiles = (g.ntiles + SORT_SEGS - 1) / SORT_SEGS;
  uint32_t *a = reinterpret_cast<uint32_t *>(data), *b = reinterpret_cast<uint32_t *>(tmp);
  uint32_t *tab = (uint32_t *)table.p, *seg = (uint32_t *)segsum.p;
  const dim3 grid((unsigned)g.ntiles, (unsigned)ncol), scan_grid(SORT_SEGS, (unsigned)ncol);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    {
      ProfScope ps(ctx, KK_SORT_HIST);
      if (pass == 0)
        hipLaunchKernelGGL(sort_hist_kernel<true>, grid, dim3(SORT_THREADS), 0, ctx->stream, a, tab, g, shift);
      else
        hipLaunchKernelGGL(sort_hist_kernel<false>, grid, dim3(SORT_THREADS), 0, ctx->stream, a, tab, g, shift);
    }
    {
      ProfScope ps(ctx, KK_SORT_SCAN);
      hipLaunchKernelGGL(sort_segsum_kernel, scan_grid, dim3(SORT_THREADS), 0, ctx->stream, tab, seg, g);
      hipLaunchKernelGGL(sort_scan_kernel, scan_grid, dim3(SORT_THREADS), 0, ctx->stream, tab, seg, g);
    }
    {
      ProfScope ps(ctx, KK_SORT_SCATTER);
      if (pass == 0)
        hipLaunchKernelGGL((sort_scatter_kernel<true, false>), grid, dim3(SORT_THREADS), 0, ctx->stream, a, b, tab, g, shift);
      else if (pass == 3)
        hipLaunchKernelGGL((sort_scatter_kernel<false, true>), grid, dim3(SORT_THREADS), 0, ctx->stream, a, b, tab, g, shift);
      else
        hipLaunchKernelGGL((sort_scatter_kernel<false, false>), grid, dim3(SORT_THREADS), 0, ctx->stream, a, b, tab, g, shift);
    }
    std::swap(a, b);
  }
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

template <typename T>
int edges_columns(ife_ctx *ctx, const T *cols, int64_t stride, int64_t n, int ncol, int nbins,
                  T *d_edges, int *d_status) {
  ProfScope ps(ctx, KK_EDGES);
  hipLaunchKernelGGL(equalized_edges_kernel<T>, dim3((unsigned)ncol), dim3(64), 0, ctx->stream, cols,
                     stride, n, nbins, d_edges, d_status);
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

int edge_status_to_rc(ife_ctx *ctx, int st, int col, int64_t n, int nbins) {
  if (st == 1)
    return fail(ctx, IFE_E_ARG,
                "Too many bins. Number of bins must be less or equal to number of samples "
                "(column %d: %lld samples, %d bins)", col, (long long)n, nbins);
  if (st == 3)
    return fail(ctx, IFE_E_STATE,
                "column %d: the edge walk ran past the last sample (%lld samples, %d bins; "
                "the reference asserts here)", col, (long long)n, nbins);
  return IFE_OK;
}

int samples_reserve(ife_samples *s, int64_t need) {
  ife_ctx *ctx = s->ctx;
  if (need <= s->cap) return IFE_OK;
  const int64_t cap = std::max<int64_t>({need, 2 * s->cap, 4096});
  DevBuf nd;  // frees itself where a step below fails
  IFE_HIP(ctx, nd.grow((size_t)cap * s->ncol * 4));
  for (int c = 0; c < s->ncol; ++c)
    if (s->count[c] > 0)
      IFE_HIP(ctx, hipMemcpyAsync((float *)nd.p + (size_t)c * cap, (float *)s->data.p + (size_t)c * s->cap,
                                  (size_t)s->count[c] * 4, hipMemcpyDeviceToDevice, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  IFE_HIP(ctx, s->data.reset());
  IFE_HIP(ctx, s->tmp.reset());
  s->data = std::move(nd);
  s->cap = cap;
  return IFE_OK;
}

// The exclusive scan of nseg segment counts, in place: [8-byte counter][nseg counts][nchunks chunk
// sums], seg_scan_bytes() rounded to 16 for what a caller keeps behind.  The caller's code kernel writes
// the counts, seg_scan() follows under the same ProfScope, scan_total() reads the counter back (blocks).
int64_t seg_scan_chunks(int64_t nseg) { return (nseg + SCAN_CHUNK - 1) / SCAN_CHUNK; }
size_t seg_scan_bytes(int64_t nseg) { return (8 + (size_t)(nseg + seg_scan_chunks(nseg)) * 4 + 15) / 16 * 16; }
uint32_t *seg_counts(const DevBuf &b) { return (uint32_t *)((char *)b.p + 8); }
int seg_scan(ife_ctx *ctx, const DevBuf &b, int64_t nseg) {
  const int64_t nchunks = seg_scan_chunks(nseg);
  uint32_t *segs = seg_counts(b), *sums = segs + nseg;
  hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)nchunks), dim3(SORT_THREADS), 0, ctx->stream, segs, nseg, sums);
  hipLaunchKernelGGL(scan_chunks_kernel, dim3(1), dim3(SORT_THREADS), 0, ctx->stream, sums, (int)nchunks,
                     (unsigned long long *)b.p);
  hipLaunchKernelGGL(chunk_scan_kernel, dim3((unsigned)nchunks), dim3(SORT_THREADS), 0, ctx->stream, segs, nseg, sums);
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}
int scan_total(ife_ctx *ctx, const DevBuf &b, int64_t *total) {
  unsigned long long h = 0;
  IFE_HIP(ctx, hipMemcpyAsync(&h, b.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *total = (int64_t)h;
  return IFE_OK;
}

template <typename TM>
int add_features_typed(ife_ctx *ctx, ife_samples *s, int first, const float *dF, int layout, int ncomp,
                       const TM *dM, int64_t nvox, const uint32_t *fg, int n_fg, const int64_t *dIdx,
                       int64_t n_idx) {
  GatherArgs a;
  a.nvox = nvox;
  a.feat_comp_stride = layout == IFE_PLANAR ? nvox : 1;
  a.feat_vox_stride = layout == IFE_PLANAR ? 1 : ncomp;
  a.ncomp = ncomp;
  a.nfg = n_fg;
  for (int k = 0; k < GATHER_MAX_FG; ++k) a.fg[k] = k < n_fg ? fg[k] : 0u;
  const int64_t have = s->count[first];
  for (int c = 1; c < ncomp; ++c)
    if (s->count[first + c] != have)
      return fail(ctx, IFE_E_STATE, "columns %d..%d hold different numbers of samples", first, first + ncomp - 1);
  if (nvox >= ((int64_t)1 << 32) - GATHER_CHUNK) return fail(ctx, IFE_E_SIZE, "volume too large for 32-bit sample offsets");
  const int nchunks = (int)((nvox + GATHER_CHUNK - 1) / GATHER_CHUNK);
  int rc = ensure(ctx, s->counter, 8 + (size_t)nchunks * 4);
  if (rc) return rc;
  unsigned long long *ctr = (unsigned long long *)s->counter.p;
  uint32_t *chunks = seg_counts(s->counter);  // here one count per chunk: only their scan is needed
  int64_t add = n_idx;
  if (!dIdx) {
    {
      ProfScope ps(ctx, KK_GATHER);
      hipLaunchKernelGGL(count_foreground_kernel<TM>, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, dM, a, chunks);
      hipLaunchKernelGGL(scan_chunks_kernel, dim3(1), dim3(SORT_THREADS), 0, ctx->stream, chunks, nchunks, ctr);
    }
    if ((rc = scan_total(ctx, s->counter, &add))) return rc;
  }
  if (add == 0) return IFE_OK;
  if ((rc = samples_reserve(s, have + add))) return rc;
  a.col_stride = s->cap;
  a.col_offset = have;
  float *cols = (float *)s->data.p + (size_t)first * s->cap;
  {
    ProfScope ps(ctx, KK_GATHER);
    if (!dIdx) {
      hipLaunchKernelGGL(gather_foreground_kernel<TM>, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, dF, dM, cols, a, chunks);
    } else {
      const unsigned b2 = (unsigned)std::min<int64_t>((n_idx + 255) / 256, 4096);
      hipLaunchKernelGGL(gather_indexed_kernel, dim3(b2), dim3(256), 0, ctx->stream, dF, dIdx, n_idx, cols, a);
    }
  }
  IFE_HIP(ctx, hipGetLastError());
  for (int c = 0; c < ncomp; ++c) s->count[first + c] = have + add;
  s->sorted = false;
  return IFE_OK;
}

int check_rois(ife_ctx *ctx, const ife_volume_desc *vol, const int64_t *rois, int n_rois) {
  if (n_rois < 1 || !rois) return fail(ctx, IFE_E_ARG, "at least one region of interest is required");
  for (int r = 0; r < n_rois; ++r) {
    const int64_t *q = rois + 6 * r;
    if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0 || q[4] < 0 || q[5] < 0 || q[0] + q[3] > vol->nx ||
        q[1] + q[4] > vol->ny || q[2] + q[5] > vol->nz)
      return fail(ctx, IFE_E_ARG,
                  "region %d [%lld, %lld, %lld][%lld, %lld, %lld] is outside of the largest possible region "
                  "[%lld, %lld, %lld]", r, (long long)q[0], (long long)q[1], (long long)q[2], (long long)q[3],
                  (long long)q[4], (long long)q[5], (long long)vol->nx, (long long)vol->ny, (long long)vol->nz);
  }
  return IFE_OK;
}

// counts (device, zeroed by the caller) += bins of every box; everything on the device
int launch_roi_histograms(ife_ctx *ctx, const float *dF, int layout, int ncomp, const void *dM, int mask_dtype,
                          const ife_volume_desc *vol, const int64_t *dRois, int n_rois, const float *dEdges,
                          int n_edges, uint32_t *dCounts) {
  RoiArgs a;
  a.nx = vol->nx; a.ny = vol->ny; a.nz = vol->nz;
  const int64_t nvox = vol->nx * vol->ny * vol->nz;
  a.feat_comp_stride = layout == IFE_PLANAR ? nvox : 1;
  a.feat_vox_stride = layout == IFE_PLANAR ? 1 : ncomp;
  a.ncomp = ncomp;
  a.nedges = n_edges;
  ProfScope ps(ctx, KK_HIST);
  const dim3 grid((unsigned)n_rois, ROI_SPLIT);
  return with_mask_type(true, mask_dtype, dM, [&](auto msk) -> int {
    using TM = std::remove_cv_t<std::remove_pointer_t<decltype(msk)>>;
    hipLaunchKernelGGL(roi_histogram_kernel<TM>, grid, dim3(256), 0, ctx->stream, dF, msk, dRois, dEdges, dCounts, a);
    IFE_HIP(ctx, hipGetLastError());
    return IFE_OK;
  });
}

// labels to {0, 1} (tool :147-152, MakeBag :236-244)
int launch_clamp01(ife_ctx *ctx, const void *dM, int mask_dtype, uint8_t *clamp, int64_t nvox) {
  const unsigned blocks = (unsigned)std::min<int64_t>((nvox + 255) / 256, 8192);
  return with_mask_type(true, mask_dtype, dM, [&](auto msk) -> int {
    using TM = std::remove_cv_t<std::remove_pointer_t<decltype(msk)>>;
    hipLaunchKernelGGL(clamp01_kernel<TM>, dim3(blocks), dim3(256), 0, ctx->stream, msk, clamp, nvox);
    IFE_HIP(ctx, hipGetLastError());
    return IFE_OK;
  });
}

int check_fg(ife_ctx *ctx, const uint32_t *fg, int n_fg, const void *idx) {
  if (idx) return IFE_OK;
  if (!fg || n_fg < 1 || n_fg > GATHER_MAX_FG)
    return fail(ctx, IFE_E_ARG, "between 1 and %d foreground values are required", GATHER_MAX_FG);
  return IFE_OK;
}

}  // namespace

// ---- determineEdgesForEqualizedHistogram (header :21-26) -------------------------------------
template <typename T>
static int equalized_edges_typed(ife_ctx *ctx, const T *sorted, int64_t n, int nbins, T *edges, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (n < 0) return fail(ctx, IFE_E_ARG, "Iterator first must come before iterator last");
  if (nbins < 1) return fail(ctx, IFE_E_ARG, "at least one bin is required");
  if (n < nbins) return edge_status_to_rc(ctx, 1, 0, n, nbins);
  if (nbins == 1) return IFE_OK;
  if (!sorted || !edges) return fail(ctx, IFE_E_ARG, "null pointer");
  const void *dS;
  if ((rc = stage_in(ctx, mem, sorted, (size_t)n * sizeof(T), ctx->st_img, &dS))) return rc;
  if ((rc = ensure(ctx, ctx->st_aux, (size_t)nbins * sizeof(T)))) return rc;
  if ((rc = ensure(ctx, ctx->st_mask, 16))) return rc;
  T *dE = mem == IFE_MEM_DEVICE ? edges : (T *)ctx->st_aux.p;
  int *dSt = (int *)ctx->st_mask.p;
  if ((rc = edges_columns<T>(ctx, (const T *)dS, n, n, 1, nbins, dE, dSt))) return rc;
  int st = 0;
  IFE_HIP(ctx, hipMemcpyAsync(&st, dSt, 4, hipMemcpyDeviceToHost, ctx->stream));
  if (mem == IFE_MEM_HOST)
    IFE_HIP(ctx, hipMemcpyAsync(edges, dE, (size_t)(nbins - 1) * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return edge_status_to_rc(ctx, st, 0, n, nbins);
}
extern "C" {

// ---- std::sort of one column (tool :284) ----------------------------------------------------
int ife_sort_f32(ife_ctx *ctx, const float *in, int64_t n, float *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, IFE_E_ARG, "null pointer");
  if (n == 0) return IFE_OK;
  void *dO;
  if ((rc = stage_out_begin(ctx, mem, out, (size_t)n * 4, &dO))) return rc;
  IFE_HIP(ctx, hipMemcpyAsync(dO, in, (size_t)n * 4,
                              mem == IFE_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                              ctx->stream));
  if ((rc = ensure(ctx, ctx->st_aux, (size_t)n * 4))) return rc;
  if ((rc = sort_columns(ctx, (float *)dO, (float *)ctx->st_aux.p, ctx->st_img, ctx->st_mask, 1, n, n)))
    return rc;
  return stage_out_end(ctx, mem, out, (size_t)n * 4);
}

// determineEdgesForEqualizedHistogram on floats / doubles
int ife_equalized_edges_f32(ife_ctx *ctx, const float *sorted, int64_t n, int nbins, float *edges,
                            int mem) {
  return equalized_edges_typed<float>(ctx, sorted, n, nbins, edges, mem);
}
int ife_equalized_edges_f64(ife_ctx *ctx, const double *sorted, int64_t n, int nbins, double *edges,
                            int mem) {
  return equalized_edges_typed<double>(ctx, sorted, n, nbins, edges, mem);
}

// ---- DenseHistogram<float> counts (DenseHistogram.h:47-53, 62-64) ----------------------------
int ife_dense_histogram_f32(ife_ctx *ctx, const float *edges, int n_edges, const float *values,
                            int64_t n, uint32_t *counts, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!edges || !counts || (n > 0 && !values)) return fail(ctx, IFE_E_ARG, "null pointer");
  if (n_edges < 1 || n_edges > HIST_MAX_EDGES)
    return fail(ctx, IFE_E_ARG, "between 1 and %d edges are required", HIST_MAX_EDGES);
  if (n < 0) return fail(ctx, IFE_E_ARG, "negative count");
  const void *dE, *dV;
  void *dC;
  if ((rc = stage_in(ctx, mem, edges, (size_t)n_edges * 4, ctx->st_mask, &dE))) return rc;
  if ((rc = stage_in(ctx, mem, n ? values : nullptr, (size_t)n * 4, ctx->st_img, &dV))) return rc;
  if ((rc = stage_out_begin(ctx, mem, counts, (size_t)(n_edges + 1) * 4, &dC))) return rc;
  IFE_HIP(ctx, hipMemsetAsync(dC, 0, (size_t)(n_edges + 1) * 4, ctx->stream));
  if (n > 0) {
    ProfScope ps(ctx, KK_HIST);
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(dense_histogram_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const float *)dE,
                       n_edges, (const float *)dV, n, (unsigned int *)dC);
    IFE_HIP(ctx, hipGetLastError());
  }
  return stage_out_end(ctx, mem, counts, (size_t)(n_edges + 1) * 4);
}

// ---- per-ROI histograms: the bag rows of tools/MakeBag.cxx:405-472 for one feature volume -----
int ife_roi_histograms(ife_ctx *ctx, const float *features, int layout, int ncomp, const void *mask,
                       int mask_dtype, const ife_volume_desc *vol, const int64_t *rois, int n_rois,
                       const float *edges, int n_edges, uint32_t *counts, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_layout_mem(ctx, layout, mem))) return rc;
  if (!features || !mask || !edges || !counts) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, false))) return rc;
  if (ncomp < 1 || n_edges < 1 || (int64_t)ncomp * (2 * n_edges + 1) > ROI_MAX_LDS_WORDS)
    return fail(ctx, IFE_E_ARG, "ncomp * (2 * n_edges + 1) must be between 3 and %d", ROI_MAX_LDS_WORDS);
  if (mem == IFE_MEM_HOST && (rc = check_rois(ctx, vol, rois, n_rois))) return rc;
  if (mem == IFE_MEM_DEVICE && (n_rois < 1 || !rois)) return fail(ctx, IFE_E_ARG, "at least one region of interest is required");
  const size_t nvox = (size_t)(vol->nx * vol->ny * vol->nz);
  const size_t cbytes = (size_t)n_rois * ncomp * (n_edges + 1) * 4;
  const void *dF, *dM, *dR, *dE;
  void *dC;
  DevBuf &aux = ctx->st_aux;
  if ((rc = stage_in(ctx, mem, features, nvox * ncomp * 4, ctx->st_img, &dF))) return rc;
  if ((rc = stage_in(ctx, mem, mask, nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
  if (mem == IFE_MEM_HOST) {  // rois and edges share one small staging buffer
    const size_t rb = (size_t)n_rois * 48, eb = (size_t)ncomp * n_edges * 4;
    if ((rc = ensure(ctx, aux, rb + eb))) return rc;
    IFE_HIP(ctx, hipMemcpyAsync(aux.p, rois, rb, hipMemcpyHostToDevice, ctx->stream));
    IFE_HIP(ctx, hipMemcpyAsync((char *)aux.p + rb, edges, eb, hipMemcpyHostToDevice, ctx->stream));
    dR = aux.p;
    dE = (char *)aux.p + rb;
  } else {
    dR = rois;
    dE = edges;
  }
  if ((rc = stage_out_begin(ctx, mem, counts, cbytes, &dC))) return rc;
  IFE_HIP(ctx, hipMemsetAsync(dC, 0, cbytes, ctx->stream));
  if ((rc = launch_roi_histograms(ctx, (const float *)dF, layout, ncomp, dM, mask_dtype, vol, (const int64_t *)dR,
                                  n_rois, (const float *)dE, n_edges, (uint32_t *)dC)))
    return rc;
  return stage_out_end(ctx, mem, counts, cbytes);
}

// one image of MakeBag (:236-244 clamp, :405-472 loop): a5 at every scale with the features
// left in HBM; counts[(roi * n_sigmas*8 + scale*8 + feature) * (n_edges+1) + bin], HOST array
int ife_bag_image(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                  const ife_volume_desc *vol, const float *sigmas, int n_sigmas, const int64_t *rois,
                  int n_rois, const float *edges, int n_edges, uint32_t *counts, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, true))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!image || !mask || !sigmas || !edges || !counts) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_sigmas(ctx, sigmas, n_sigmas))) return rc;
  if ((rc = check_image_dtype(ctx, image_dtype))) return rc;
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, false))) return rc;
  if (n_edges < 1 || (int64_t)IFE_NUM_FEATURES * (2 * n_edges + 1) > ROI_MAX_LDS_WORDS)
    return fail(ctx, IFE_E_ARG, "between 1 and %d edges per histogram", (ROI_MAX_LDS_WORDS / IFE_NUM_FEATURES - 1) / 2);
  if ((rc = check_rois(ctx, vol, rois, n_rois))) return rc;  // rois, edges and counts are host arrays
  const size_t nvox = (size_t)(vol->nx * vol->ny * vol->nz);
  const int ncol = n_sigmas * IFE_NUM_FEATURES, nb = n_edges + 1;
  const void *dI, *dM;
  if ((rc = stage_in(ctx, mem, image, nvox * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, mask, nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
  const size_t rb = (size_t)n_rois * 48, eb = (size_t)ncol * n_edges * 4, cb = (size_t)n_rois * ncol * nb * 4;
  const size_t off_e = rb, off_c = (rb + eb + 15) / 16 * 16, off_m = off_c + (cb + 15) / 16 * 16;
  const size_t off_f = off_m + (nvox + 15) / 16 * 16;
  if ((rc = ensure(ctx, ctx->st_aux, off_f + nvox * IFE_NUM_FEATURES * n_sigmas * 4))) return rc;
  char *ws = (char *)ctx->st_aux.p;
  IFE_HIP(ctx, hipMemcpyAsync(ws, rois, rb, hipMemcpyHostToDevice, ctx->stream));
  IFE_HIP(ctx, hipMemcpyAsync(ws + off_e, edges, eb, hipMemcpyHostToDevice, ctx->stream));
  IFE_HIP(ctx, hipMemsetAsync(ws + off_c, 0, cb, ctx->stream));
  uint8_t *clamp = (uint8_t *)(ws + off_m);
  float *feat = (float *)(ws + off_f);
  if ((rc = launch_clamp01(ctx, dM, mask_dtype, clamp, (int64_t)nvox))) return rc;
  // IFE_OPT_DIFFERENTIAL: the same buffer from the jet
  if ((rc = feature_volumes(ctx, dI, image_dtype, clamp, IFE_U8, vol, sigmas, n_sigmas, feat, IFE_PLANAR,
                            ctx->differential != 0)))
    return rc;
  // per scale: counts of that scale's 8 histograms for every box, laid out [roi][scale*8+k][bin]
  // through a per-scale scratch [roi][8][bin] and a strided copy back
  std::vector<uint32_t> tmp((size_t)n_rois * IFE_NUM_FEATURES * nb);
  for (int i = 0; i < n_sigmas; ++i) {
    uint32_t *dC = (uint32_t *)(ws + off_c);
    IFE_HIP(ctx, hipMemsetAsync(dC, 0, tmp.size() * 4, ctx->stream));
    if ((rc = launch_roi_histograms(ctx, feat + (size_t)i * nvox * IFE_NUM_FEATURES, IFE_PLANAR, IFE_NUM_FEATURES,
                                    clamp, IFE_U8, vol, (const int64_t *)ws,
                                    n_rois, (const float *)(ws + off_e) + (size_t)i * IFE_NUM_FEATURES * n_edges,
                                    n_edges, dC)))
      return rc;
    IFE_HIP(ctx, hipMemcpyAsync(tmp.data(), dC, tmp.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < n_rois; ++r)
      memcpy(counts + ((size_t)r * ncol + (size_t)i * IFE_NUM_FEATURES) * nb,
             tmp.data() + (size_t)r * IFE_NUM_FEATURES * nb, (size_t)IFE_NUM_FEATURES * nb * 4);
  }
  return IFE_OK;
}

// ---- the sample columns of the tool (:165-166) ------------------------------------------------
int ife_samples_create(ife_ctx *ctx, int n_columns, ife_samples **out) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!out) return fail(ctx, IFE_E_ARG, "samples out pointer is null");
  *out = nullptr;
  if (n_columns < 1 || n_columns > 4096) return fail(ctx, IFE_E_ARG, "1..4096 columns");
  ife_samples *s = new (std::nothrow) ife_samples();
  if (!s) return fail(ctx, IFE_E_NOMEM, "host allocation failed");
  s->ctx = ctx;
  s->ncol = n_columns;
  s->count.assign(n_columns, 0);
  *out = s;
  return IFE_OK;
}

void ife_samples_destroy(ife_samples *s) {
  if (!s) return;
  (void)hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);
  delete s;  // its DevBufs free themselves
}

int ife_samples_count(const ife_samples *s, int column, int64_t *n) {
  if (!s || !n || column < 0 || column >= s->ncol) return IFE_E_ARG;
  *n = s->count[column];
  return IFE_OK;
}

int ife_samples_clear(ife_samples *s) {
  if (!s) return IFE_E_ARG;
  std::fill(s->count.begin(), s->count.end(), 0);
  s->sorted = false;
  return IFE_OK;
}

// append the features of the accepted voxels of one scale to columns [first, first+ncomp)
int ife_samples_add_features(ife_ctx *ctx, ife_samples *s, int first_column, const float *features,
                             int layout, int ncomp, const void *mask, int mask_dtype, int64_t nvox,
                             const uint32_t *foreground, int n_foreground, const int64_t *indices,
                             int64_t n_indices, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!s || s->ctx != ctx) return fail(ctx, IFE_E_ARG, "samples object does not belong to this context");
  if ((rc = check_layout_mem(ctx, layout, mem))) return rc;
  if (ncomp < 1 || first_column < 0 || first_column + ncomp > s->ncol)
    return fail(ctx, IFE_E_ARG, "columns %d..%d out of range (0..%d)", first_column,
                first_column + ncomp - 1, s->ncol - 1);
  if (!features || nvox < 1) return fail(ctx, IFE_E_ARG, "null pointer");
  if (!indices && !mask) return fail(ctx, IFE_E_ARG, "a mask or a list of voxel indices is required");
  if ((rc = check_fg(ctx, foreground, n_foreground, indices))) return rc;
  if (indices) {
    if (n_indices < 0) return fail(ctx, IFE_E_ARG, "negative count");
    if (mem == IFE_MEM_HOST)
      for (int64_t k = 0; k < n_indices; ++k)
        if (indices[k] < 0 || indices[k] >= nvox) return fail(ctx, IFE_E_ARG, "voxel index out of range");
  } else if ((rc = check_mask_dtype(ctx, mask, mask_dtype, false))) {
    return rc;
  }
  const void *dF, *dM = nullptr, *dI = nullptr;
  if ((rc = stage_in(ctx, mem, features, (size_t)nvox * ncomp * 4, ctx->st_img, &dF))) return rc;
  if (indices) {
    if ((rc = stage_in(ctx, mem, indices, (size_t)n_indices * 8, ctx->st_aux, &dI))) return rc;
  } else if ((rc = stage_in(ctx, mem, mask, (size_t)nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) {
    return rc;
  }
  return with_mask_type(!indices, mask_dtype, dM, [&](auto msk) {  // the indexed form reads no mask
    return add_features_typed(ctx, s, first_column, (const float *)dF, layout, ncomp, msk, nvox, foreground,
                              n_foreground, (const int64_t *)dI, n_indices);
  });
}

// one image of the tool's loop (:176-265): clamp the labels to {0,1} (:147-152), a5 at
// every scale with the features left in HBM, samples of scale i into columns [8i, 8i+8)
int ife_samples_add_image(ife_ctx *ctx, ife_samples *s, const void *image, int image_dtype,
                          const void *mask, int mask_dtype, const ife_volume_desc *vol,
                          const float *sigmas, int n_sigmas, const uint32_t *foreground,
                          int n_foreground, const int64_t *indices, int64_t n_indices_per_scale,
                          int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!s || s->ctx != ctx) return fail(ctx, IFE_E_ARG, "samples object does not belong to this context");
  if ((rc = check_vol(ctx, vol, true))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!image || !mask || !sigmas) return fail(ctx, IFE_E_ARG, "null pointer");
  if (n_sigmas < 1 || n_sigmas * IFE_NUM_FEATURES != s->ncol)
    return fail(ctx, IFE_E_ARG, "the samples object has %d columns, %d scales need %d", s->ncol, n_sigmas,
                n_sigmas * IFE_NUM_FEATURES);
  if ((rc = check_sigmas(ctx, sigmas, n_sigmas))) return rc;
  if ((rc = check_image_dtype(ctx, image_dtype))) return rc;
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, false))) return rc;
  if ((rc = check_fg(ctx, foreground, n_foreground, indices))) return rc;
  const int64_t nvox = vol->nx * vol->ny * vol->nz;
  if (indices) {
    if (n_indices_per_scale < 0) return fail(ctx, IFE_E_ARG, "negative count");
    if (mem == IFE_MEM_HOST)
      for (int64_t k = 0; k < n_indices_per_scale * n_sigmas; ++k)
        if (indices[k] < 0 || indices[k] >= nvox) return fail(ctx, IFE_E_ARG, "voxel index out of range");
  }
  const void *dI, *dM, *dIdx = nullptr;
  if ((rc = stage_in(ctx, mem, image, (size_t)nvox * dtype_size(image_dtype), ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, mask, (size_t)nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
  if (indices && (rc = stage_in(ctx, mem, indices, (size_t)n_indices_per_scale * n_sigmas * 8, s->idx, &dIdx)))
    return rc;
  if ((rc = ensure(ctx, s->clamp, (size_t)nvox))) return rc;
  if ((rc = launch_clamp01(ctx, dM, mask_dtype, (uint8_t *)s->clamp.p, nvox))) return rc;
  const bool differential = ctx->differential != 0;
  if (!dIdx) {
    // all-foreground branch, fused: the feature kernel writes the eight features of every
    // sampled voxel straight into the columns (raster order); no feature volume exists
    // (IFE_OPT_DIFFERENTIAL: straight from the jet instead, whose workspace is its own)
    if ((rc = reserve_scales(ctx, vol, differential))) return rc;
    for (int c = 1; c < s->ncol; ++c)
      if (s->count[c] != s->count[0]) return fail(ctx, IFE_E_STATE, "columns hold different numbers of samples");
    GatherArgs a;
    a.nvox = nvox;
    a.nfg = n_foreground;
    for (int k = 0; k < GATHER_MAX_FG; ++k) a.fg[k] = k < n_foreground ? foreground[k] : 0u;
    const int gx = (int)((vol->nx + 63) / 64);
    const int64_t nseg = (int64_t)gx * vol->ny * vol->nz;
    if (nseg >= ((int64_t)1 << 31)) return fail(ctx, IFE_E_SIZE, "volume too large for the segment table");
    // the scan of the per-segment sample counts is 32 bits wide: a dense foreground on 2^32 or
    // more voxels would wrap it and misplace samples silently (the gather branch refuses the same)
    if (nvox >= ((int64_t)1 << 32))
      return fail(ctx, IFE_E_SIZE, "volume too large for 32-bit sample offsets");
    if ((rc = ensure(ctx, s->feat, (size_t)nvox))) return rc;                 // the per-voxel code
    if ((rc = ensure(ctx, s->counter, seg_scan_bytes(nseg)))) return rc;
    uint8_t *code = (uint8_t *)s->feat.p;
    uint32_t *segs = seg_counts(s->counter);
    {
      ProfScope ps(ctx, KK_GATHER);
      const unsigned sb = (unsigned)std::min<int64_t>((nseg + 3) / 4, 32768);
      with_mask_type(true, mask_dtype, dM, [&](auto msk) {
        using TM = std::remove_cv_t<std::remove_pointer_t<decltype(msk)>>;
        hipLaunchKernelGGL(sample_code_kernel<TM>, dim3(sb), dim3(256), 0, ctx->stream, msk, code, segs,
                           (int)vol->nx, gx, nseg, a);
        return IFE_OK;
      });
      if ((rc = seg_scan(ctx, s->counter, nseg))) return rc;
    }
    int64_t h = 0;
    if ((rc = scan_total(ctx, s->counter, &h))) return rc;
    if (h == 0) return IFE_OK;
    const int64_t have = s->count[0];
    if ((rc = samples_reserve(s, have + h))) return rc;
    const ColumnSink sink = {code, segs, (float *)s->data.p, s->cap, have, gx, nseg};
    rc = with_types(image_dtype, dI, true, IFE_U8, s->clamp.p, [&](auto img, auto cm) {
      return feature_scales(ctx, img, cm, vol, sigmas, n_sigmas, differential, sink, nullptr);
    });
    if (rc) return rc;
    for (int c = 0; c < s->ncol; ++c) s->count[c] = have + h;
    s->sorted = false;
    return IFE_OK;
  }
  // sampled branch: the listed voxels are read from a feature volume left in HBM
  if ((rc = ensure(ctx, s->feat, (size_t)nvox * IFE_NUM_FEATURES * n_sigmas * 4))) return rc;
  if ((rc = feature_volumes(ctx, dI, image_dtype, s->clamp.p, IFE_U8, vol, sigmas, n_sigmas, (float *)s->feat.p,
                            IFE_PLANAR, differential)))
    return rc;
  for (int i = 0; i < n_sigmas && !rc; ++i) {
    const float *f = (const float *)s->feat.p + (size_t)i * nvox * IFE_NUM_FEATURES;
    const int64_t *ix = (const int64_t *)dIdx + (size_t)i * n_indices_per_scale;
    rc = add_features_typed(ctx, s, i * IFE_NUM_FEATURES, f, IFE_PLANAR, IFE_NUM_FEATURES, (const uint8_t *)dM, nvox,
                            foreground, n_foreground, ix, n_indices_per_scale);
  }
  return rc;
}

// sort every column (in place, once)
int ife_samples_sort(ife_ctx *ctx, ife_samples *s) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!s || s->ctx != ctx) return fail(ctx, IFE_E_ARG, "samples object does not belong to this context");
  if (s->sorted) return IFE_OK;
  if (s->cap > 0 && (rc = ensure(ctx, s->tmp, (size_t)s->cap * s->ncol * 4))) return rc;
  // columns with equal counts go through the passes together
  for (int c0 = 0; c0 < s->ncol;) {
    int c1 = c0 + 1;
    while (c1 < s->ncol && s->count[c1] == s->count[c0]) ++c1;
    if ((rc = sort_columns(ctx, (float *)s->data.p + (size_t)c0 * s->cap, (float *)s->tmp.p + (size_t)c0 * s->cap,
                           s->table, s->totals, c1 - c0, s->count[c0], s->cap)))
      return rc;
    c0 = c1;
  }
  s->sorted = true;
  return IFE_OK;
}

// tool :282-289: sort, then the equalizing edges of every column; edges is a host array of
// n_columns * (nbins - 1) floats, column-major rows as the tool writes them
int ife_samples_equalized_edges(ife_ctx *ctx, ife_samples *s, int nbins, float *edges) {
  int rc = ife_samples_sort(ctx, s);
  if (rc) return rc;
  if (nbins < 1) return fail(ctx, IFE_E_ARG, "at least one bin is required");
  for (int c = 0; c < s->ncol; ++c)
    if (s->count[c] < nbins) return edge_status_to_rc(ctx, 1, c, s->count[c], nbins);
  if (nbins == 1) return IFE_OK;
  if (!edges) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = ensure(ctx, s->edges, (size_t)s->ncol * (nbins - 1) * 4))) return rc;
  if ((rc = ensure(ctx, s->status, (size_t)s->ncol * 4))) return rc;
  for (int c0 = 0; c0 < s->ncol;) {
    int c1 = c0 + 1;
    while (c1 < s->ncol && s->count[c1] == s->count[c0]) ++c1;
    if ((rc = edges_columns<float>(ctx, (const float *)s->data.p + (size_t)c0 * s->cap, s->cap, s->count[c0], c1 - c0,
                            nbins, (float *)s->edges.p + (size_t)c0 * (nbins - 1), (int *)s->status.p + c0)))
      return rc;
    c0 = c1;
  }
  std::vector<int> st(s->ncol);
  IFE_HIP(ctx, hipMemcpyAsync(st.data(), s->status.p, (size_t)s->ncol * 4, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipMemcpyAsync(edges, s->edges.p, (size_t)s->ncol * (nbins - 1) * 4, hipMemcpyDeviceToHost,
                              ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int c = 0; c < s->ncol; ++c)
    if ((rc = edge_status_to_rc(ctx, st[c], c, s->count[c], nbins))) return rc;
  return IFE_OK;
}

// copy one column to the host (tests, and tools that want the samples themselves)
int ife_samples_read_column(ife_ctx *ctx, const ife_samples *s, int column, float *out, int64_t capacity) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!s || s->ctx != ctx || column < 0 || column >= s->ncol || !out)
    return fail(ctx, IFE_E_ARG, "bad samples object, column or pointer");
  if (capacity < s->count[column]) return fail(ctx, IFE_E_ARG, "output holds %lld values, the column %lld",
                                              (long long)capacity, (long long)s->count[column]);
  if (s->count[column] == 0) return IFE_OK;
  IFE_HIP(ctx, hipMemcpyAsync(out, (const float *)s->data.p + (size_t)column * s->cap,
                              (size_t)s->count[column] * 4, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return IFE_OK;
}

}  // extern "C"
