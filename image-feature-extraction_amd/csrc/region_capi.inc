// region_capi.inc -- ife_mask_bounding_box, ife_extract_region and ife_label_membership of
// include/ife_hip.h (DESIGN.md "Regions"); included at the end of ife_capi.hip.  The checks and
// the per-axis split of the extract are region_plan.hpp's, plain host code.

namespace {

// element count times element size of a volume, or -1 where that does not fit 2^62
int64_t region_volume_bytes(const ife_volume_desc *v, int64_t elem_bytes) {
  const int64_t plane = v->nx * v->ny;  // each below 2^31
  if (v->nz > (((int64_t)1 << 62) / elem_bytes) / plane) return -1;
  return plane * v->nz * elem_bytes;
}

bool region_ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

template <int ES, bool FLOATBITS>
void launch_region_box(ife_ctx *ctx, const void *dM, const ife_volume_desc *vol, RegionBoxRecord *rec) {
  const int64_t nrows = vol->ny * vol->nz, row_bytes = vol->nx * ES;
  const int64_t per = std::max<int64_t>(1, std::min<int64_t>(REGION_BOX_UNIT_BYTES / row_bytes, nrows));
  const int64_t nunits = (nrows + per - 1) / per;
  const unsigned blocks = (unsigned)std::min<int64_t>(nunits, REGION_BOX_GRID_CAP);
  hipLaunchKernelGGL((region_box_kernel<ES, FLOATBITS>), dim3(blocks), dim3(REGION_BLOCK), 0, ctx->stream,
                     (const unsigned char *)dM, (uint32_t)vol->nx, (uint32_t)vol->ny, nrows, per, nunits, rec);
}

template <int ES>
void launch_region_extract(ife_ctx *ctx, const void *dS, void *dD, const RegionExtractArgs &g, bool flipx) {
  const int64_t nrows = g.out_n[1] * g.out_n[2];
  const unsigned blocks =
      (unsigned)std::min<int64_t>((nrows + REGION_WAVES - 1) / REGION_WAVES, REGION_EXTRACT_GRID_CAP);
  if (flipx)
    hipLaunchKernelGGL((region_extract_kernel<ES, true>), dim3(blocks), dim3(REGION_BLOCK), 0, ctx->stream,
                       (const unsigned char *)dS, (unsigned char *)dD, g, nrows);
  else
    hipLaunchKernelGGL((region_extract_kernel<ES, false>), dim3(blocks), dim3(REGION_BLOCK), 0, ctx->stream,
                       (const unsigned char *)dS, (unsigned char *)dD, g, nrows);
}

template <typename T>
void launch_region_member(ife_ctx *ctx, const void *dL, int64_t n, const uint32_t *dBits, int inside, int outside,
                          void *dO) {
  const int64_t pieces = n / (16 / (int64_t)sizeof(T)) + 1;
  const unsigned blocks =
      (unsigned)std::min<int64_t>((pieces + REGION_BLOCK - 1) / REGION_BLOCK, REGION_MEMBER_GRID_CAP);
  hipLaunchKernelGGL(region_member_kernel<T>, dim3(blocks), dim3(REGION_BLOCK), 0, ctx->stream, (const T *)dL, n,
                     dBits, (T)inside, (T)outside, (T *)dO);
}

}  // namespace

extern "C" {

// ---- the tightest box around the foreground and the number of foreground voxels ------------------
int ife_mask_bounding_box(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol, int64_t box[6],
                          int64_t *count, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, false))) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (mask_dtype != IFE_U8 && mask_dtype != IFE_U16 && mask_dtype != IFE_I16 && mask_dtype != IFE_F32)
    return fail(ctx, IFE_E_ARG, "mask dtype must be IFE_U8, IFE_U16, IFE_I16 or IFE_F32");
  if (!mask || !box || !count) return fail(ctx, IFE_E_ARG, "null pointer");
  const int64_t es = (int64_t)dtype_size(mask_dtype);
  if (mem == IFE_MEM_DEVICE && reinterpret_cast<uintptr_t>(mask) % es)
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  const int64_t bytes = region_volume_bytes(vol, es);
  if (bytes < 0) return fail(ctx, IFE_E_SIZE, "the volume's byte count overflows");
  const void *dM;
  if ((rc = stage_in(ctx, mem, mask, (size_t)bytes, ctx->st_mask, &dM))) return rc;
  if ((rc = ensure(ctx, ctx->st_aux, sizeof(RegionBoxRecord)))) return rc;
  RegionBoxRecord *dRec = (RegionBoxRecord *)ctx->st_aux.p;
  IFE_HIP(ctx, hipMemsetAsync(dRec->lo, 0xff, sizeof dRec->lo, ctx->stream));
  IFE_HIP(ctx, hipMemsetAsync(dRec->hi, 0, sizeof(RegionBoxRecord) - sizeof dRec->lo, ctx->stream));
  {
    ProfScope ps(ctx, KK_MASK);
    if (mask_dtype == IFE_U8) launch_region_box<1, false>(ctx, dM, vol, dRec);
    else if (mask_dtype == IFE_F32) launch_region_box<4, true>(ctx, dM, vol, dRec);
    else launch_region_box<2, false>(ctx, dM, vol, dRec);
    IFE_HIP(ctx, hipGetLastError());
  }
  RegionBoxRecord rec;
  IFE_HIP(ctx, hipMemcpyAsync(&rec, dRec, sizeof rec, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *count = (int64_t)rec.count;
  for (int a = 0; a < 3; ++a) {
    box[a] = rec.count ? (int64_t)rec.lo[a] : 0;
    box[3 + a] = rec.count ? (int64_t)rec.hi[a] - (int64_t)rec.lo[a] + 1 : 0;
  }
  return IFE_OK;
}

// ---- crop, pad and flip in one gather ----------------------------------------------------------------
int ife_extract_region(ife_ctx *ctx, const void *src, int elem_bytes, const ife_volume_desc *src_vol,
                       const int64_t region[6], int flip, const void *pad_value, void *dst, int src_mem,
                       int dst_mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, src_vol, false))) return rc;
  if ((rc = check_mem(ctx, src_mem)) || (rc = check_mem(ctx, dst_mem))) return rc;
  const int64_t n_src[3] = {src_vol->nx, src_vol->ny, src_vol->nz};
  RegionPlan plan;
  const char *msg = "";
  if ((rc = region_check(elem_bytes, n_src, region, flip, pad_value != nullptr, &plan, &msg)))
    return fail(ctx, rc == REGION_E_SIZE ? IFE_E_SIZE : IFE_E_ARG, "%s", msg);
  if (!src || !dst) return fail(ctx, IFE_E_ARG, "null pointer");
  const int64_t src_bytes = region_volume_bytes(src_vol, elem_bytes);
  if (src_bytes < 0) return fail(ctx, IFE_E_SIZE, "the source's byte count overflows");
  const int64_t dst_bytes = region[3] * region[4] * region[5] * elem_bytes;  // at most 2^40: region_check
  if ((src_mem == IFE_MEM_DEVICE && reinterpret_cast<uintptr_t>(src) % elem_bytes) ||
      (dst_mem == IFE_MEM_DEVICE && reinterpret_cast<uintptr_t>(dst) % elem_bytes))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  if (src_mem == IFE_MEM_DEVICE && dst_mem == IFE_MEM_DEVICE &&
      region_ranges_overlap(src, (size_t)src_bytes, dst, (size_t)dst_bytes))
    return fail(ctx, IFE_E_ARG, "src and dst overlap");
  RegionExtractArgs g;
  for (int a = 0; a < 3; ++a) {
    g.ax[a] = plan.ax[a];
    g.out_n[a] = region[3 + a];
  }
  g.src_nx = src_vol->nx;
  g.src_ny = src_vol->ny;
  unsigned char pad[16] = {0};
  if (pad_value)
    for (int i = 0; i < 16; i += elem_bytes) std::memcpy(pad + i, pad_value, (size_t)elem_bytes);
  std::memcpy(&g.pad, pad, 16);
  const void *dS = src;  // a region of pad only reads no source: nothing is staged for it
  if (!plan.all_pad && (rc = stage_in(ctx, src_mem, src, (size_t)src_bytes, ctx->st_img, &dS))) return rc;
  void *dD;
  if ((rc = stage_out_begin(ctx, dst_mem, dst, (size_t)dst_bytes, &dD))) return rc;
  {
    ProfScope ps(ctx, KK_GATHER);
    const bool flipx = (flip & 1) != 0;
    switch (elem_bytes) {
      case 1: launch_region_extract<1>(ctx, dS, dD, g, flipx); break;
      case 2: launch_region_extract<2>(ctx, dS, dD, g, flipx); break;
      case 4: launch_region_extract<4>(ctx, dS, dD, g, flipx); break;
      default: launch_region_extract<8>(ctx, dS, dD, g, flipx); break;
    }
    IFE_HIP(ctx, hipGetLastError());
  }
  if (dst_mem == IFE_MEM_DEVICE) {  // the call blocks in every mode: a staged source may be reused
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IFE_OK;
  }
  return stage_out_end(ctx, dst_mem, dst, (size_t)dst_bytes);
}

// ---- tools/ExtractMaskedRegion.cxx:62-67: inside where the label is in the set, else outside -------
int ife_label_membership(ife_ctx *ctx, const void *labels, int labels_dtype, int64_t n, const int *include,
                         int n_include, int inside, int outside, void *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (labels_dtype != IFE_U8 && labels_dtype != IFE_U16)
    return fail(ctx, IFE_E_ARG, "labels dtype must be IFE_U8 or IFE_U16");
  const int top = labels_dtype == IFE_U8 ? 255 : 65535;
  if (n <= 0) return fail(ctx, IFE_E_SIZE, "element count must be positive");
  if (n > ((int64_t)1 << 40)) return fail(ctx, IFE_E_SIZE, "more than 2^40 elements");
  if (n_include < 0 || (n_include > 0 && !include) || !labels || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if (inside < 0 || inside > top || outside < 0 || outside > top)
    return fail(ctx, IFE_E_ARG, "inside and outside must lie in 0 .. %d", top);
  std::vector<uint32_t> bits((size_t)(top + 1) / 32, 0u);
  for (int i = 0; i < n_include; ++i) {
    if (include[i] < 0 || include[i] > top)
      return fail(ctx, IFE_E_ARG, "include value %d is outside 0 .. %d", include[i], top);
    bits[(size_t)include[i] >> 5] |= 1u << (include[i] & 31);
  }
  const size_t es = dtype_size(labels_dtype), bytes = (size_t)n * es;
  if (mem == IFE_MEM_DEVICE) {
    if (reinterpret_cast<uintptr_t>(labels) % es || reinterpret_cast<uintptr_t>(out) % es)
      return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
    if (region_ranges_overlap(labels, bytes, out, bytes)) return fail(ctx, IFE_E_ARG, "labels and out overlap");
  }
  const void *dL;
  void *dO;
  if ((rc = stage_in(ctx, mem, labels, bytes, ctx->st_img, &dL))) return rc;
  if ((rc = ensure(ctx, ctx->st_aux, bits.size() * 4))) return rc;
  IFE_HIP(ctx, hipMemcpyAsync(ctx->st_aux.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = stage_out_begin(ctx, mem, out, bytes, &dO))) return rc;
  {
    ProfScope ps(ctx, KK_MASK);
    if (labels_dtype == IFE_U8)
      launch_region_member<uint8_t>(ctx, dL, n, (const uint32_t *)ctx->st_aux.p, inside, outside, dO);
    else
      launch_region_member<uint16_t>(ctx, dL, n, (const uint32_t *)ctx->st_aux.p, inside, outside, dO);
    IFE_HIP(ctx, hipGetLastError());
  }
  if (mem == IFE_MEM_DEVICE) {  // the bitmap was copied from a vector of this frame
    IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IFE_OK;
  }
  return stage_out_end(ctx, mem, out, bytes);
}

// ---- device buffers for callers without a HIP runtime of their own -----------------------------------
int ife_device_alloc(ife_ctx *ctx, size_t bytes, void **ptr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!ptr || bytes == 0) return fail(ctx, IFE_E_ARG, "null pointer or no bytes");
  *ptr = nullptr;
  IFE_HIP(ctx, hipMalloc(ptr, bytes));
  return IFE_OK;
}

int ife_device_upload(ife_ctx *ctx, void *dst, const void *src, size_t bytes) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!dst || !src || bytes == 0) return fail(ctx, IFE_E_ARG, "null pointer or no bytes");
  IFE_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return IFE_OK;
}

int ife_device_free(ife_ctx *ctx, void *ptr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!ptr) return IFE_OK;
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  IFE_HIP(ctx, hipFree(ptr));
  return IFE_OK;
}

}  // extern "C"
