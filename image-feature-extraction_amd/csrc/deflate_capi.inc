// deflate_capi.inc -- DEFLATE blocks formed on the device (deflate_kernels.hpp): ife_deflate and
// the deflated fetch of the scale stream (include/ife_hip.h).  Included at the end of ife_capi.hip
// behind scales_capi.inc, whose stream it reads.
//
// Two passes, so that nothing of the size of the input is staged: the size pass leaves a byte
// count and a CRC piece per chunk, a scan turns the counts into offsets, the total is read back
// and held against the capacity, and only then the emit pass stores -- every store inside
// [offset, offset + count) of its chunk, so none can pass the end of the output.  These kernels
// are not booked in the kernel-time table (its kinds are part of the ABI).

namespace {

// What the passes leave in ctx->df_ws for nchunks chunks: offsets, then the total and the CRC
// pieces next to each other (one copy brings both to the host), then the byte counts.
struct DeflateWs {
  uint64_t *offsets, *total;
  uint32_t *crcs, *sizes;
  static size_t bytes(size_t nchunks) { return (nchunks + 1) * 8 + nchunks * 8; }
  DeflateWs(void *p, size_t nchunks)
      : offsets((uint64_t *)p), total(offsets + nchunks), crcs((uint32_t *)(total + 1)), sizes(crcs + nchunks) {}
};

size_t deflate_chunks(size_t bytes) { return (bytes + DF_CHUNK - 1) / DF_CHUNK; }

// Size pass and scan over `bytes` device bytes on `stream`; waits for them.  *total: the size of
// the blocks, *crc: the CRC-32 of the input.
int deflate_sizes(ife_ctx *ctx, hipStream_t stream, const void *din, size_t bytes, size_t *total, uint32_t *crc) {
  const size_t nchunks = deflate_chunks(bytes);
  if (nchunks > 0x7fffffffu) return fail(ctx, IFE_E_SIZE, "more than 2^31-1 chunks of %d bytes", DF_CHUNK);
  *total = 0;
  *crc = 0;
  if (nchunks == 0) return IFE_OK;
  int rc = ensure(ctx, ctx->df_ws, DeflateWs::bytes(nchunks));
  if (rc) return rc;
  const DeflateWs ws(ctx->df_ws.p, nchunks);
  hipLaunchKernelGGL(df_chunk_kernel<false>, dim3((unsigned)nchunks), dim3(DF_THREADS), 0, stream,
                     (const uint8_t *)din, (uint64_t)bytes, ws.sizes, ws.crcs, (const uint64_t *)nullptr,
                     (uint8_t *)nullptr);
  IFE_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(df_scan_kernel, dim3(1), dim3(DF_THREADS), 0, stream, (const uint32_t *)ws.sizes,
                     (int64_t)nchunks, ws.offsets, ws.total);
  IFE_HIP(ctx, hipGetLastError());
  std::vector<uint32_t> host(2 + nchunks);
  IFE_HIP(ctx, hipMemcpyAsync(host.data(), ws.total, host.size() * 4, hipMemcpyDeviceToHost, stream));
  IFE_HIP(ctx, hipStreamSynchronize(stream));
  uint64_t t;
  memcpy(&t, host.data(), 8);
  *total = (size_t)t;
  *crc = df_fold_crc(host.data() + 2, nchunks, bytes);
  return IFE_OK;
}

// Emit pass behind deflate_sizes of the same input: the blocks to dout (device), which holds the
// total that deflate_sizes returned.  Enqueued on `stream`.
int deflate_emit(ife_ctx *ctx, hipStream_t stream, const void *din, size_t bytes, void *dout) {
  const size_t nchunks = deflate_chunks(bytes);
  if (nchunks == 0) return IFE_OK;
  const DeflateWs ws(ctx->df_ws.p, nchunks);
  hipLaunchKernelGGL(df_chunk_kernel<true>, dim3((unsigned)nchunks), dim3(DF_THREADS), 0, stream,
                     (const uint8_t *)din, (uint64_t)bytes, (uint32_t *)nullptr, (uint32_t *)nullptr,
                     (const uint64_t *)ws.offsets, (uint8_t *)dout);
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

int deflate_too_small(ife_ctx *ctx, size_t total, size_t capacity) {
  return fail(ctx, IFE_E_SIZE, "the blocks take %zu bytes, the output holds %zu", total, capacity);
}

}  // namespace

extern "C" {

size_t ife_deflate_bound(size_t bytes) { return bytes + 5 * deflate_chunks(bytes); }

int ife_deflate(ife_ctx *ctx, const void *data, size_t bytes, void *out, size_t capacity, size_t *out_bytes,
                uint32_t *crc32, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_mem(ctx, mem))) return rc;
  if (!data || !out || !out_bytes || !crc32) return fail(ctx, IFE_E_ARG, "null pointer");
  if (bytes == 0) {
    *out_bytes = 0;
    *crc32 = 0;
    return IFE_OK;
  }
  const void *dI;
  if ((rc = stage_in(ctx, mem, data, bytes, ctx->st_img, &dI))) return rc;
  if ((rc = deflate_sizes(ctx, ctx->stream, dI, bytes, out_bytes, crc32))) return rc;
  if (*out_bytes > capacity) return deflate_too_small(ctx, *out_bytes, capacity);
  void *dO;
  if ((rc = stage_out_begin(ctx, mem, out, *out_bytes, &dO))) return rc;
  if ((rc = deflate_emit(ctx, ctx->stream, dI, bytes, dO))) return rc;
  if (mem == IFE_MEM_HOST) return stage_out_end(ctx, mem, out, *out_bytes);
  IFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return IFE_OK;
}

int ife_emphysema_features_fetch_deflated(ife_ctx *ctx, int scale, int component, void *out, size_t capacity,
                                          size_t *out_bytes, uint32_t *crc32) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!out || !out_bytes || !crc32) return fail(ctx, IFE_E_ARG, "null pointer");
  if (scale < 0 || scale >= (int)ctx->sc_done.size())
    return fail(ctx, IFE_E_STATE, "scale %d was not started by ife_emphysema_features_begin (%d scales)",
                scale, (int)ctx->sc_done.size());
  if (ctx->sc_layout != IFE_PLANAR)
    return fail(ctx, IFE_E_STATE, "the components of an interleaved stream are not contiguous: begin it with IFE_PLANAR");
  if (component < 0 || component >= IFE_NUM_FEATURES)
    return fail(ctx, IFE_E_ARG, "component %d out of range (0..%d)", component, IFE_NUM_FEATURES - 1);
  const size_t plane = ctx->sc_scale_bytes / IFE_NUM_FEATURES;
  const char *src = (const char *)ctx->sc_out.p + (size_t)scale * ctx->sc_scale_bytes + (size_t)component * plane;
  IFE_HIP(ctx, hipStreamWaitEvent(ctx->sc_copy, ctx->sc_done[scale], 0));
  if ((rc = deflate_sizes(ctx, ctx->sc_copy, src, plane, out_bytes, crc32))) return rc;
  if (*out_bytes > capacity) return deflate_too_small(ctx, *out_bytes, capacity);
  if (ctx->df_out.cap < *out_bytes) {
    // nothing uses the old buffer: every call that filled it has waited for its copy.  A quarter
    // of the plane at least, so that planes of the usual density do not make it grow again
    // (freeing device memory waits for the scales that are still running).
    IFE_HIP(ctx, ctx->df_out.grow(std::max(*out_bytes, ife_deflate_bound(plane) / 4)));
  }
  if ((rc = deflate_emit(ctx, ctx->sc_copy, src, plane, ctx->df_out.p))) return rc;
  if (*out_bytes)
    IFE_HIP(ctx, hipMemcpyAsync(out, ctx->df_out.p, *out_bytes, hipMemcpyDeviceToHost, ctx->sc_copy));
  IFE_HIP(ctx, hipStreamSynchronize(ctx->sc_copy));
  return IFE_OK;
}

}  // extern "C"
