// distance_capi.inc -- entry points of SURVEY.md section 2 row 8 (include/ife_hip.h): the signed
// Maurer distance map and the expected distance; included at the end of ife_capi.hip (shares
// its context, staging and profiling helpers).

namespace {

// Blocks of the y / z pass (one lane per line); the candidate stacks hold n entries per lane
unsigned edt_line_blocks(int64_t nlines) {
  return (unsigned)std::min<int64_t>((nlines + 63) / 64, EDT_MAX_LINE_BLOCKS);
}

// The three passes on device memory.  map != nullptr: the signed map is built in place in `map`.
// map == nullptr: the unsquared inside-positive map is reduced with `prob` over the foreground
// on the fly; result[0] = mean, result[1] = count (as int64 bits), both in ctx->edt_part.
template <typename TM>
int edt_run(ife_ctx *ctx, const TM *mask, const ife_volume_desc *vol, int positive, int squared, double *map,
            const double *prob) {
  const int64_t nx = vol->nx, ny = vol->ny, nz = vol->nz;
  if (nx > EDT_MAX_NX)
    return fail(ctx, IFE_E_SIZE, "the distance map takes at most %lld voxels along x", (long long)EDT_MAX_NX);
  const size_t nvox = (size_t)(nx * ny * nz);
  const unsigned by = edt_line_blocks(nx * nz), bz = edt_line_blocks(nx * ny);
  const size_t entries = std::max((size_t)ny * by, (size_t)nz * bz) * 64;
  int rc = ensure(ctx, ctx->edt_g, entries * sizeof(double));
  if (!rc) rc = ensure(ctx, ctx->edt_i, entries * sizeof(int32_t));
  if (rc) return rc;
  double *d2 = map, *psum = nullptr, *result = nullptr;
  uint32_t *pcnt = nullptr;
  if (!map) {
    // the squared map, then per z line a partial sum and a count, then the two result words
    const size_t nl = (size_t)(nx * ny), off_c = 16 + nl * 8;
    if ((rc = ensure(ctx, ctx->edt_d2, nvox * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->edt_part, off_c + nl * 4))) return rc;
    d2 = (double *)ctx->edt_d2.p;
    result = (double *)ctx->edt_part.p;
    psum = result + 2;
    pcnt = (uint32_t *)((char *)ctx->edt_part.p + off_c);
  }
  EdtLines a;
  a.ws_g = (double *)ctx->edt_g.p;
  a.ws_i = (int32_t *)ctx->edt_i.p;
  {
    ProfScope ps(ctx, KK_EDT_X);
    const unsigned blocks = (unsigned)std::min<int64_t>(ny * nz, 1 << 20);
    hipLaunchKernelGGL(edt_x_kernel<TM>, dim3(blocks), dim3(64), 0, ctx->stream, mask, d2, nx, ny, nz, vol->sx);
  }
  {
    ProfScope ps(ctx, KK_EDT_Y);
    a.nlines = nx * nz; a.inner = nx; a.outer = nx * ny; a.stride = nx; a.n = (int)ny; a.spacing = vol->sy;
    hipLaunchKernelGGL((edt_line_kernel<TM, 0>), dim3(by), dim3(64), 0, ctx->stream, d2, a, mask, 0, 0,
                       (double *)nullptr, (const double *)nullptr, (double *)nullptr, (uint32_t *)nullptr);
  }
  {
    ProfScope ps(ctx, KK_EDT_Z);
    a.nlines = nx * ny; a.inner = nx * ny; a.outer = 0; a.stride = nx * ny; a.n = (int)nz; a.spacing = vol->sz;
    if (map)
      hipLaunchKernelGGL((edt_line_kernel<TM, 1>), dim3(bz), dim3(64), 0, ctx->stream, d2, a, mask, positive, squared,
                         map, (const double *)nullptr, (double *)nullptr, (uint32_t *)nullptr);
    else
      hipLaunchKernelGGL((edt_line_kernel<TM, 2>), dim3(bz), dim3(64), 0, ctx->stream, d2, a, mask, 1, 0,
                         (double *)nullptr, prob, psum, pcnt);
  }
  if (!map) {
    ProfScope ps(ctx, KK_EDT_REDUCE);
    hipLaunchKernelGGL(edt_reduce_kernel, dim3(1), dim3(EDT_REDUCE_THREADS), 0, ctx->stream, psum, pcnt, nx * ny,
                       result);
  }
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

// checks common to both entry points; `field` is the double volume that follows `mem`
int edt_check(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol, const void *field,
              int mem) {
  int rc = check_vol(ctx, vol, false);
  if (rc) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!field) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, false))) return rc;
  if (mem == IFE_MEM_DEVICE && (reinterpret_cast<uintptr_t>(field) % 8 ||
                                reinterpret_cast<uintptr_t>(mask) % dtype_size(mask_dtype)))
    return fail(ctx, IFE_E_ARG, "device pointers must be aligned to their element size");
  return IFE_OK;
}

}  // namespace

extern "C" {

// ---- itk::SignedMaurerDistanceMapImageFilter (header :16-19) ---------------------------------
int ife_signed_distance_map(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol,
                            int inside_is_positive, int squared, double *out, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = edt_check(ctx, mask, mask_dtype, vol, out, mem))) return rc;
  const size_t nvox = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dM;
  void *dO;
  if ((rc = stage_in(ctx, mem, mask, nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out, nvox * 8, &dO))) return rc;
  rc = with_mask_type(true, mask_dtype, dM, [&](auto msk) {
    return edt_run(ctx, msk, vol, inside_is_positive, squared, (double *)dO, nullptr);
  });
  if (rc) return rc;
  return stage_out_end(ctx, mem, out, nvox * 8);
}

// ---- expectedDistanceFromCenterToInterestPoint (header :9-43) --------------------------------
int ife_expected_distance(ife_ctx *ctx, const void *mask, int mask_dtype, const double *prob,
                          const ife_volume_desc *vol, double *result, int64_t *n_inside, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = edt_check(ctx, mask, mask_dtype, vol, prob, mem))) return rc;
  if (!result) return fail(ctx, IFE_E_ARG, "null pointer");
  const size_t nvox = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dM, *dP;
  if ((rc = stage_in(ctx, mem, mask, nvox * dtype_size(mask_dtype), ctx->st_mask, &dM))) return rc;
  if ((rc = stage_in(ctx, mem, prob, nvox * 8, ctx->st_img, &dP))) return rc;
  rc = with_mask_type(true, mask_dtype, dM, [&](auto msk) {
    return edt_run(ctx, msk, vol, 1, 0, (double *)nullptr, (const double *)dP);
  });
  if (rc) return rc;
  double h[2];
  IFE_HIP(ctx, hipMemcpyAsync(h, ctx->edt_part.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *result = h[0];
  if (n_inside) memcpy(n_inside, &h[1], 8);
  return IFE_OK;
}

}  // extern "C"
