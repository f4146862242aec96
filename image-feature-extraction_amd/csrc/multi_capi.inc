// multi_capi.inc -- one process, several devices: the Z-slab decomposition of the feature
// path (DESIGN.md section 6) driven from C++ with peer copies over xGMI.
//
// Same decomposition, kernels and schedule as image-feature-extraction_amd/slab.py (which
// runs one process per GPU over RCCL): rank r of W owns a contiguous range of planes; the Z
// recursion crosses slab boundaries as 32-byte state records (ife_stage_z_sweep for the
// direction whose state reaches a rank first, ife_stage_z_fused for the other; every slab of the
// raw data is uploaded with the neighbours' adjacent planes, IFE_Z_OVERLAP_LO below and _HI
// above, so the input history of a state never travels), the last axis pass stores the quotient
// (ife_stage_recursive_gaussian_quotient) and the stencil needs one boundary plane of that
// smoothed value per scale from each neighbour.  Here one host thread enqueues everything: every "rank" is a
// pair of ife_ctx (bulk stream, high-priority chain stream) on its device, transfers are
// hipMemcpyPeerAsync on the sender's stream, and every dependency is a HIP event recorded
// before it is waited for -- the chain items are enqueued in wavefront order (causal item i
// at rank r in step r + i, anticausal in step W-1-r + i), so no wait can refer to an event
// that has not been recorded.  The same device may appear more than once in the list (that
// is how the tests exercise W > 1 on a one-GPU box); the reference has no counterpart
// (SURVEY.md section 8e).  The differential path (ife_multi_differential_features) runs the same
// slabs, uploads and state chains with six Z jobs per scale and nothing but slab-local work behind
// them (multi_run, MultiPath).  Included by ife_capi.hip.

namespace {

struct MultiRank {
  int dev = 0;
  ife_ctx *bulk = nullptr, *chain = nullptr;
  hipStream_t sb = nullptr, sc = nullptr, sd = nullptr;  // bulk, boundary chain, downloads
  int64_t z0 = 0, nzl = 0;
  int64_t lo = 0, hi = 0;  // planes of the neighbours carried below / above the slab's own
  DevBuf img, mask, src[2], out;
  std::vector<DevBuf> zo, xo, pad, ck;        // [scale * nf + field]
  std::vector<DevBuf> c_in, c_out, a_in, a_out;  // [item]
  std::vector<hipEvent_t> ev;                  // every event of a run, destroyed at its end
  hipEvent_t uploaded = nullptr;               // behind the run's uploads from host memory (one of ev)
};

}  // namespace

struct ife_multi {
  std::vector<MultiRank> ranks;
  std::string err;
  int trig_mode = -1;  // -1: the library default
  // streaming form (ife_multi_emphysema_features_begin / _fetch / _end): the geometry of the
  // call in flight and, per rank and scale, the event behind that scale's feature launch
  bool streaming = false;
  ife_volume_desc s_vol = {0, 0, 0, 1.0, 1.0, 1.0};
  int s_scales = 0, s_layout = 0;
  std::vector<std::vector<hipEvent_t>> s_done;  // [rank][scale]
};

namespace {

int mfail(ife_multi *m, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (m) m->err = buf;
  else g_create_error = buf;
  return code;
}

#define IFE_MHIP(m, call)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return mfail(m, e_ == hipErrorOutOfMemory ? IFE_E_NOMEM : IFE_E_HIP, "%s: %s", #call,    \
                   hipGetErrorString(e_));                                                     \
  } while (0)

int mensure(ife_multi *m, MultiRank &R, DevBuf &b, size_t bytes) {
  if (b.cap >= bytes) return IFE_OK;
  IFE_MHIP(m, hipSetDevice(R.dev));
  IFE_MHIP(m, b.grow(bytes));
  return IFE_OK;
}

// an event recorded now on `s` (device of R current); owned by the run
int mrecord(ife_multi *m, MultiRank &R, hipStream_t s, hipEvent_t *out) {
  hipEvent_t e;
  IFE_MHIP(m, hipSetDevice(R.dev));
  IFE_MHIP(m, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  R.ev.push_back(e);
  IFE_MHIP(m, hipEventRecord(e, s));
  *out = e;
  return IFE_OK;
}
int mwait(ife_multi *m, MultiRank &R, hipStream_t s, hipEvent_t e) {
  if (!e) return IFE_OK;
  IFE_MHIP(m, hipSetDevice(R.dev));
  IFE_MHIP(m, hipStreamWaitEvent(s, e, 0));
  return IFE_OK;
}
int mcopy(ife_multi *m, MultiRank &from, hipStream_t s, MultiRank &to, void *dst, const void *src,
          size_t bytes) {
  IFE_MHIP(m, hipSetDevice(from.dev));
  if (from.dev == to.dev)
    IFE_MHIP(m, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  else
    IFE_MHIP(m, hipMemcpyPeerAsync(dst, to.dev, src, from.dev, bytes, s));
  return IFE_OK;
}

void mfree_rank(MultiRank &R) {
  (void)hipSetDevice(R.dev);
  const hipStream_t streams[3] = {R.sb, R.sc, R.sd};
  for (hipStream_t s : streams)
    if (s) (void)hipStreamSynchronize(s);
  for (auto e : R.ev) (void)hipEventDestroy(e);
  // the rank's own buffers go first (an empty rank in its place frees every DevBuf of it), then
  // its two contexts, its streams last
  ife_ctx *const bulk = R.bulk, *const chain = R.chain;
  R = MultiRank();
  if (bulk) ife_ctx_destroy(bulk);
  if (chain) ife_ctx_destroy(chain);
  for (hipStream_t s : streams)
    if (s) (void)hipStreamDestroy(s);
}

#define IFE_MCTX(m, R, c, call)                                                     \
  do {                                                                              \
    int rc_ = (call);                                                               \
    if (rc_ != IFE_OK) return mfail(m, rc_, "device %d: %s", (R).dev, ife_last_error(c)); \
  } while (0)

}  // namespace

extern "C" {

int ife_multi_create(const int *devices, int n_devices, ife_multi **out) {
  if (!out) return mfail(nullptr, IFE_E_ARG, "multi out pointer is null");
  *out = nullptr;
  if (!devices || n_devices < 1 || n_devices > 64)
    return mfail(nullptr, IFE_E_ARG, "between 1 and 64 devices are required");
  ife_multi *m = new (std::nothrow) ife_multi();
  if (!m) return mfail(nullptr, IFE_E_NOMEM, "host allocation failed");
  m->ranks.resize((size_t)n_devices);
  for (int r = 0; r < n_devices; ++r) {
    MultiRank &R = m->ranks[(size_t)r];
    R.dev = devices[r];
    int rc = ife_ctx_create(R.dev, &R.bulk);
    if (!rc) rc = ife_ctx_create(R.dev, &R.chain);
    hipError_t e = hipSuccess;
    if (!rc) {
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // hi is the numerically lowest = highest priority
      e = hipStreamCreateWithFlags(&R.sb, hipStreamNonBlocking);
      if (e == hipSuccess) e = hipStreamCreateWithPriority(&R.sc, hipStreamNonBlocking, hi);
      if (e == hipSuccess) e = hipStreamCreateWithFlags(&R.sd, hipStreamNonBlocking);
    }
    if (rc || e != hipSuccess) {
      const std::string why = rc ? ife_last_error(nullptr) : hipGetErrorString(e);
      for (auto &Q : m->ranks) mfree_rank(Q);
      delete m;
      return mfail(nullptr, rc ? rc : IFE_E_HIP, "device %d: %s", devices[r], why.c_str());
    }
    ife_ctx_set_stream(R.bulk, R.sb);
    ife_ctx_set_stream(R.chain, R.sc);
  }
  // neighbours on different devices copy peer to peer; failure to enable (already enabled, or
  // no direct path) is not fatal: hipMemcpyPeerAsync then stages through the host
  for (int r = 0; r + 1 < n_devices; ++r) {
    const int a = devices[r], b = devices[r + 1];
    if (a == b) continue;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) {
      (void)hipSetDevice(a);
      (void)hipDeviceEnablePeerAccess(b, 0);
      (void)hipSetDevice(b);
      (void)hipDeviceEnablePeerAccess(a, 0);
    }
    (void)hipGetLastError();
  }
  *out = m;
  return IFE_OK;
}

void ife_multi_destroy(ife_multi *m) {
  if (!m) return;
  for (auto &R : m->ranks) mfree_rank(R);
  delete m;
}

const char *ife_multi_last_error(const ife_multi *m) { return m ? m->err.c_str() : g_create_error.c_str(); }

int ife_multi_set_option(ife_multi *m, int option, int value) {
  if (!m) return IFE_E_ARG;
  if (option == IFE_OPT_DIFFERENTIAL && value == 1)
    return mfail(m, IFE_E_ARG, "the differential path runs on one device (IFE_OPT_DIFFERENTIAL stays 0 here)");
  for (auto &R : m->ranks) {
    IFE_MCTX(m, R, R.bulk, ife_ctx_set_option(R.bulk, option, value));
    IFE_MCTX(m, R, R.chain, ife_ctx_set_option(R.chain, option, value));
  }
  return IFE_OK;
}

}  // extern "C"

namespace {

// The feature path of a run.  Both cut the volume into the same slabs, upload them with the same
// overlap and carry the Z recursion through the same two state chains; they differ in the Z jobs
// of a scale and in what the bulk stream makes of the Z output:
//   MULTI_FD   numerator and denominator (or the image alone), order 0; then X, Y with the
//              quotient, one stencil plane from each neighbour, ife_stage_features;
//   MULTI_JET  cT and c at orders 0, 1, 2, source-major (so that the lean sweeps read every plane
//              once for its three orders); then ife_stage_jet_features, which is slab-local: no
//              plane is exchanged.  c is the constant 1.0f without a mask, as jet_sources makes it.
enum MultiPath { MULTI_FD, MULTI_JET };

// Everything a feature call enqueues; may return early with work in flight and events alive --
// the caller drains (multi_drain) whatever this returns.
int multi_run(ife_multi *m, MultiPath path, const void *image, int image_dtype, const void *mask, int mask_dtype,
              const ife_volume_desc *vol, const float *sigmas, int n_sigmas, int layout) {
  if (!vol || !image || !sigmas) return mfail(m, IFE_E_ARG, "null pointer");
  const int W = (int)m->ranks.size();
  const int64_t nx = vol->nx, ny = vol->ny, nz = vol->nz;
  // the shared checks report through the first rank's context
  ife_ctx *c0 = m->ranks[0].bulk;
  int rc;
  if ((rc = check_sigmas(c0, sigmas, n_sigmas)) || (rc = check_image_dtype(c0, image_dtype)) ||
      (rc = check_mask_dtype(c0, mask, mask_dtype, true)) || (rc = check_layout_mem(c0, layout, IFE_MEM_HOST)))
    return mfail(m, rc, "%s", c0->err.c_str());
  if (nx < 4 || ny < 4 || nz < (int64_t)4 * W)
    return mfail(m, IFE_E_SIZE, "every Z-slab needs at least 4 planes and every axis 4 voxels "
                                "(%lld x %lld x %lld over %d devices)",
                 (long long)nx, (long long)ny, (long long)nz, W);
  if ((rc = check_vol(c0, vol, false))) return mfail(m, rc, "%s", c0->err.c_str());  // spacing
  const bool jet = path == MULTI_JET;
  const int nf = mask ? 2 : 1, S = n_sigmas;
  const int nsrc = jet ? 2 : nf;  // float sources of the Z jobs
  const int jps = jet ? 6 : nf;   // Z jobs per scale: job s * jps + k * (jps / nsrc) + order
  const int64_t plane = nx * ny;
  const size_t isz = dtype_size(image_dtype), msz = mask ? dtype_size(mask_dtype) : 0;
  // slabs: nz / W planes each, the remainder spread over the first ranks
  {
    int64_t z = 0;
    for (int r = 0; r < W; ++r) {
      m->ranks[(size_t)r].z0 = z;
      m->ranks[(size_t)r].nzl = nz / W + (r < nz % W ? 1 : 0);
      m->ranks[(size_t)r].lo = r > 0 ? IFE_Z_OVERLAP_LO : 0;
      m->ranks[(size_t)r].hi = r < W - 1 ? IFE_Z_OVERLAP_HI : 0;
      z += m->ranks[(size_t)r].nzl;
    }
  }
  // chain items: (scale group, line group); groups as slab.py chooses them
  const int max_jobs = IIR_MAX_JOBS / jps;  // scales per chain item (one on the differential path)
  const int spi = std::max(1, std::min(max_jobs, S));
  std::vector<std::vector<int>> sgroups;
  for (int s0 = 0; s0 < S; s0 += spi) {
    sgroups.emplace_back();
    for (int s = s0; s < std::min(S, s0 + spi); ++s) sgroups.back().push_back(s);
  }
  int G = W == 1 ? 1 : 4;
  G = (int)std::max<int64_t>(1, std::min<int64_t>(G, (plane + 255) / 256));
  const int64_t per = ((plane + G - 1) / G + 255) / 256 * 256;
  std::vector<std::pair<int64_t, int64_t>> lgroups;
  for (int64_t l0 = 0; l0 < plane; l0 += per) lgroups.emplace_back(l0, std::min(plane, l0 + per) - l0);
  struct Item { int q, g; };
  std::vector<Item> items;
  for (int q = 0; q < (int)sgroups.size(); ++q)
    for (int g = 0; g < (int)lgroups.size(); ++g) items.push_back(Item{q, g});
  const int NI = (int)items.size();
  // bulk groups: the first scale group alone, the rest merged up to max_jobs jobs per launch
  std::vector<std::vector<int>> bgroups(1, std::vector<int>(1, 0));
  for (int q = 1; q < (int)sgroups.size(); ++q) {
    size_t n_sc = sgroups[(size_t)q].size();
    for (int k : bgroups.back()) n_sc += sgroups[(size_t)k].size();
    if (bgroups.size() > 1 && (int)n_sc <= max_jobs) bgroups.back().push_back(q);
    else bgroups.emplace_back(1, q);
  }

  if (getenv("IFE_MULTI_TRACE"))  // one line per upload + prepass: the host-tool tests count them
    fprintf(stderr, "ife_multi: upload and prepass of %lld x %lld x %lld over %d devices, %d scales\n",
            (long long)nx, (long long)ny, (long long)nz, W, S);
  // ---- buffers, inputs ------------------------------------------------------------------
  for (int r = 0; r < W; ++r) {
    MultiRank &R = m->ranks[(size_t)r];
    const size_t nvl = (size_t)(R.nzl * plane);
    const size_t nve = (size_t)((R.lo + R.nzl + R.hi) * plane);  // with the neighbours' planes
    ife_volume_desc slab = {nx, ny, R.nzl, vol->sx, vol->sy, vol->sz};
    int rc = mensure(m, R, R.img, nve * isz);
    if (!rc && mask) rc = mensure(m, R, R.mask, nve * msz);
    for (int k = 0; k < nsrc && !rc; ++k) rc = mensure(m, R, R.src[k], (nve + 3) / 4 * 16);  // whole 16-byte pieces
    if (!rc) rc = mensure(m, R, R.out, nvl * IFE_NUM_FEATURES * 4 * (size_t)S);
    // (never shrunk: an engine that runs both paths in turn keeps the buffers of both)
    R.zo.resize(std::max(R.zo.size(), (size_t)(S * jps))); R.xo.resize(std::max(R.xo.size(), (size_t)(S * nf)));
    R.pad.resize(std::max(R.pad.size(), (size_t)S)); R.ck.resize(std::max(R.ck.size(), (size_t)(S * jps)));
    for (int j = 0; j < S * jps && !rc; ++j) {
      rc = mensure(m, R, R.zo[(size_t)j], nvl * 4);
      if (!rc) rc = mensure(m, R, R.ck[(size_t)j], ife_stage_z_ck_bytes(&slab));
    }
    for (int j = 0; j < S * nf && !rc && !jet; ++j) rc = mensure(m, R, R.xo[(size_t)j], nvl * 4);
    for (int j = 0; j < S && !rc && !jet; ++j)  // the smoothed value of a scale with one halo plane each side
      rc = mensure(m, R, R.pad[(size_t)j], (size_t)((R.nzl + 2) * plane) * 4);
    const size_t ni = std::max(R.c_in.size(), (size_t)NI);
    R.c_in.resize(ni); R.c_out.resize(ni); R.a_in.resize(ni); R.a_out.resize(ni);
    for (int i = 0; i < NI && !rc; ++i) {
      const size_t sb = sgroups[(size_t)items[(size_t)i].q].size() * (size_t)jps * IFE_Z_STATE_BYTES *
                        (size_t)lgroups[(size_t)items[(size_t)i].g].second;
      rc = mensure(m, R, R.c_in[(size_t)i], sb);
      if (!rc) rc = mensure(m, R, R.c_out[(size_t)i], sb);
      if (!rc) rc = mensure(m, R, R.a_in[(size_t)i], sb);
      if (!rc) rc = mensure(m, R, R.a_out[(size_t)i], sb);
    }
    if (rc) return rc;
    IFE_MHIP(m, hipSetDevice(R.dev));
    IFE_MHIP(m, hipMemcpyAsync(R.img.p, (const char *)image + (size_t)((R.z0 - R.lo) * plane) * isz, nve * isz,
                               hipMemcpyHostToDevice, R.sb));
    if (mask)
      IFE_MHIP(m, hipMemcpyAsync(R.mask.p, (const char *)mask + (size_t)((R.z0 - R.lo) * plane) * msz, nve * msz,
                                 hipMemcpyHostToDevice, R.sb));
    if ((rc = mrecord(m, R, R.sb, &R.uploaded))) return rc;
  }

  // ---- prepare, then the two state chains in wavefront order -----------------------------
  std::vector<hipEvent_t> prepared((size_t)W, nullptr);
  for (int r = 0; r < W; ++r) {
    MultiRank &R = m->ranks[(size_t)r];
    ife_volume_desc ext = {nx, ny, R.lo + R.nzl + R.hi, vol->sx, vol->sy, vol->sz};  // the prepass covers the overlap
    IFE_MCTX(m, R, R.bulk, ife_stage_prepare(R.bulk, R.img.p, image_dtype, mask ? R.mask.p : nullptr, mask_dtype,
                                             &ext, 1, (float *)R.src[0].p, mask ? (float *)R.src[1].p : nullptr));
    if (jet && !mask) {  // certainty one everywhere: the second source is the constant
      const int64_t n4 = ((R.lo + R.nzl + R.hi) * plane + 3) / 4;
      const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 0x7fffffff);
      IFE_MHIP(m, hipSetDevice(R.dev));
      hipLaunchKernelGGL(stream_fill_kernel, dim3(blocks), dim3(256), 0, R.sb, (float4 *)R.src[1].p, n4, 1.0f);
      IFE_MHIP(m, hipGetLastError());
    }
    int rc = mrecord(m, R, R.sb, &prepared[(size_t)r]);
    if (!rc) rc = mwait(m, R, R.sc, prepared[(size_t)r]);
    if (rc) return rc;
  }
  // arrived[d][r][i]: the incoming state of item i, direction d, has landed in rank r's buffer
  std::vector<std::vector<std::vector<hipEvent_t>>> arrived(
      2, std::vector<std::vector<hipEvent_t>>((size_t)W, std::vector<hipEvent_t>((size_t)NI, nullptr)));
  auto swept = arrived;  // swept[d][r][i]: the sweep has run (checkpoints are in place)
  for (int t = 0; t < NI + W - 1; ++t) {
    for (int r = 0; r < W; ++r) {
      MultiRank &R = m->ranks[(size_t)r];
      ife_volume_desc slab = {nx, ny, R.nzl, vol->sx, vol->sy, vol->sz};
      for (int d = 0; d < 2; ++d) {
        const int i = d == 0 ? t - r : t - (W - 1 - r);
        if (i < 0 || i >= NI) continue;
        const std::vector<int> &ss = sgroups[(size_t)items[(size_t)i].q];
        const int64_t l0 = lgroups[(size_t)items[(size_t)i].g].first, nl = lgroups[(size_t)items[(size_t)i].g].second;
        const bool has_nb = d == 0 ? r > 0 : r < W - 1;
        const float *in[IIR_MAX_JOBS];
        float *zo_w[IIR_MAX_JOBS];
        void *ck[IIR_MAX_JOBS];
        double sg[IIR_MAX_JOBS];
        int ord[IIR_MAX_JOBS];
        int nj = 0;
        for (int s : ss)
          for (int k = 0; k < jps; ++k, ++nj) {
            in[nj] = (const float *)R.src[k / (jps / nsrc)].p + R.lo * plane;  // the slab's own plane 0
            zo_w[nj] = (float *)R.zo[(size_t)(s * jps + k)].p;
            ck[nj] = R.ck[(size_t)(s * jps + k)].p;
            sg[nj] = (double)sigmas[s];
            ord[nj] = k % (jps / nsrc);
          }
        const int *orders = jet ? ord : nullptr;
        int rc = has_nb ? mwait(m, R, R.sc, arrived[(size_t)d][(size_t)r][(size_t)i]) : IFE_OK;
        if (rc) return rc;
        DevBuf &sin = d == 0 ? R.c_in[(size_t)i] : R.a_in[(size_t)i];
        DevBuf &sout = d == 0 ? R.c_out[(size_t)i] : R.a_out[(size_t)i];
        // the direction whose state reaches this rank first is a lean sweep, the other one is
        // carried through the slab together with the combine (slab.py, SlabEngine.lean)
        const int lean = r <= W - 1 - r ? 0 : 1;
        if (d == lean) {
          IFE_MCTX(m, R, R.chain, ife_stage_z_sweep_order(R.chain, d, nj, in, &slab, l0, nl, sg, orders, has_nb ? 1 : 0,
                                                          has_nb ? sin.p : nullptr, sout.p, ck));
        } else {
          IFE_MCTX(m, R, R.chain, ife_stage_z_fused_order(R.chain, d, nj, in, zo_w, &slab, l0, nl, sg, orders, r > 0,
                                                          r < W - 1, has_nb ? sin.p : nullptr, sout.p, ck));
        }
        if ((rc = mrecord(m, R, R.sc, &swept[(size_t)d][(size_t)r][(size_t)i]))) return rc;
        const int nb = d == 0 ? r + 1 : r - 1;
        if (nb >= 0 && nb < W) {
          MultiRank &N = m->ranks[(size_t)nb];
          DevBuf &dst = d == 0 ? N.c_in[(size_t)i] : N.a_in[(size_t)i];
          if ((rc = mcopy(m, R, R.sc, N, dst.p, sout.p, (size_t)nj * IFE_Z_STATE_BYTES * (size_t)nl))) return rc;
          if ((rc = mrecord(m, R, R.sc, &arrived[(size_t)d][(size_t)nb][(size_t)i]))) return rc;
        }
      }
    }
  }

  // ---- bulk: X, Y (quotient), stencil planes, features, per bulk group ------------------------
  const size_t pb = (size_t)plane * 4;
  m->s_done.assign((size_t)W, std::vector<hipEvent_t>((size_t)S, nullptr));
  m->s_vol = *vol;
  m->s_scales = S;
  m->s_layout = layout;
  if (jet) {
    // ---- bulk of the differential path: per scale X level, Y level and the pointwise pass, all
    // slab-local (a chain item holds one scale: scale group q is scale q) ----------------------
    for (int s = 0; s < S; ++s)
      for (int r = 0; r < W; ++r) {
        MultiRank &R = m->ranks[(size_t)r];
        ife_volume_desc slab = {nx, ny, R.nzl, vol->sx, vol->sy, vol->sz};
        const int fat = r <= W - 1 - r ? 1 : 0;
        for (int i = 0; i < NI; ++i)
          if (items[(size_t)i].q == s) {
            int rc = mwait(m, R, R.sb, swept[(size_t)fat][(size_t)r][(size_t)i]);  // the fused kernels wrote the Z output
            if (rc) return rc;
          }
        const float *zf[6];
        for (int k = 0; k < 6; ++k) zf[k] = (const float *)R.zo[(size_t)(s * 6 + k)].p;
        const void *own_mask = mask ? (const char *)R.mask.p + (size_t)(R.lo * plane) * msz : nullptr;
        const size_t scale_out = (size_t)(R.nzl * plane) * IFE_NUM_FEATURES;
        IFE_MCTX(m, R, R.bulk, ife_stage_jet_features(R.bulk, zf, own_mask, mask_dtype, &slab, (double)sigmas[s],
                                                      (float *)R.out.p + (size_t)s * scale_out, layout));
        int rc = mrecord(m, R, R.sb, &m->s_done[(size_t)r][(size_t)s]);
        if (rc) return rc;
      }
    return IFE_OK;
  }
  for (const std::vector<int> &qs : bgroups) {
    std::vector<int> ss;
    for (int q : qs) for (int s : sgroups[(size_t)q]) ss.push_back(s);
    const int nj = (int)ss.size() * nf, ns = (int)ss.size();
    for (int r = 0; r < W; ++r) {
      MultiRank &R = m->ranks[(size_t)r];
      ife_volume_desc slab = {nx, ny, R.nzl, vol->sx, vol->sy, vol->sz};
      const int fat = r <= W - 1 - r ? 1 : 0;
      for (int i = 0; i < NI; ++i)
        if (std::find(qs.begin(), qs.end(), items[(size_t)i].q) != qs.end()) {
          int rc = mwait(m, R, R.sb, swept[(size_t)fat][(size_t)r][(size_t)i]);  // the fused kernels wrote the Z output
          if (rc) return rc;
        }
      const float *zo[IIR_MAX_JOBS], *xnum[IIR_MAX_JOBS], *xden[IIR_MAX_JOBS];
      float *xo_w[IIR_MAX_JOBS], *pad1[IIR_MAX_JOBS];
      double sg[IIR_MAX_JOBS], sg1[IIR_MAX_JOBS];
      int j = 0, js = 0;
      for (int s : ss) {
        for (int k = 0; k < nf; ++k, ++j) {
          const size_t b = (size_t)(s * nf + k);
          zo[j] = (const float *)R.zo[b].p;
          xo_w[j] = (float *)R.xo[b].p;
          sg[j] = (double)sigmas[s];
        }
        xnum[js] = (const float *)R.xo[(size_t)(s * nf)].p;
        xden[js] = nf == 2 ? (const float *)R.xo[(size_t)(s * nf + 1)].p : nullptr;
        pad1[js] = (float *)R.pad[(size_t)s].p + plane;  // planes 1 .. nzl of [nzl + 2]
        sg1[js] = (double)sigmas[s];
        ++js;
      }
      IFE_MCTX(m, R, R.bulk, ife_stage_recursive_gaussian_batch(R.bulk, nj, zo, xo_w, &slab, 0, sg, 1));
      if (nf == 2)
        IFE_MCTX(m, R, R.bulk, ife_stage_recursive_gaussian_quotient(R.bulk, ns, xnum, xden, pad1, &slab, 1, sg1));
      else
        IFE_MCTX(m, R, R.bulk, ife_stage_recursive_gaussian_batch(R.bulk, ns, xnum, pad1, &slab, 1, sg1, 1));
    }
    // boundary planes of the smoothed value to the neighbours (on the sender's bulk stream,
    // behind its Y pass)
    std::vector<hipEvent_t> from_lo((size_t)W, nullptr), from_hi((size_t)W, nullptr);
    for (int r = 0; r < W; ++r) {
      MultiRank &R = m->ranks[(size_t)r];
      for (int side = 0; side < 2; ++side) {
        const int nb = side == 0 ? r - 1 : r + 1;
        if (nb < 0 || nb >= W) continue;
        MultiRank &N = m->ranks[(size_t)nb];
        for (int s : ss) {
          const char *mine = (const char *)R.pad[(size_t)s].p + (side == 0 ? pb : (size_t)R.nzl * pb);  // first / last plane
          char *theirs = (char *)N.pad[(size_t)s].p + (side == 0 ? (size_t)(N.nzl + 1) * pb : 0);        // its hi / lo halo
          int rc = mcopy(m, R, R.sb, N, theirs, mine, pb);
          if (rc) return rc;
        }
        int rc = mrecord(m, R, R.sb, side == 0 ? &from_hi[(size_t)nb] : &from_lo[(size_t)nb]);
        if (rc) return rc;
      }
    }
    for (int r = 0; r < W; ++r) {
      MultiRank &R = m->ranks[(size_t)r];
      ife_volume_desc slab = {nx, ny, R.nzl, vol->sx, vol->sy, vol->sz};
      int rc = mwait(m, R, R.sb, from_lo[(size_t)r]);
      if (!rc) rc = mwait(m, R, R.sb, from_hi[(size_t)r]);
      if (rc) return rc;
      const int lo = r > 0 ? 1 : 0, hi = r < W - 1 ? 1 : 0;
      const size_t first = lo ? 0 : (size_t)plane;  // without a lower neighbour the buffer starts at plane 1
      const size_t scale_out = (size_t)(R.nzl * plane) * IFE_NUM_FEATURES;
      for (int s : ss) {
        const float *val = (const float *)R.pad[(size_t)s].p + first;
        const void *own_mask = mask ? (const char *)R.mask.p + (size_t)(R.lo * plane) * msz : nullptr;
        IFE_MCTX(m, R, R.bulk, ife_stage_features(R.bulk, val, nullptr, own_mask, mask_dtype, &slab, lo,
                                                  hi, (float *)R.out.p + (size_t)s * scale_out, layout));
        if ((rc = mrecord(m, R, R.sb, &m->s_done[(size_t)r][(size_t)s]))) return rc;
      }
    }
  }
  return IFE_OK;
}

// The slabs of one scale back into the caller's volume (host memory), behind that scale's
// feature launches; returns with the copies enqueued on the ranks' bulk streams.
int multi_fetch_scale(ife_multi *m, int s, float *out) {
  const ife_volume_desc *vol = &m->s_vol;
  const int64_t plane = vol->nx * vol->ny, nz = vol->nz;
  const int W = (int)m->ranks.size(), layout = m->s_layout;
  for (int r = 0; r < W; ++r) {
    MultiRank &R = m->ranks[(size_t)r];
    IFE_MHIP(m, hipSetDevice(R.dev));
    const size_t slab_vox = (size_t)(R.nzl * plane);
    const float *src = (const float *)R.out.p + (size_t)s * slab_vox * IFE_NUM_FEATURES;
    // on the download stream, behind this scale's feature launch only: the later scales keep
    // the bulk stream busy meanwhile
    int rc = mwait(m, R, R.sd, m->s_done[(size_t)r][(size_t)s]);
    if (rc) return rc;
    if (layout == IFE_INTERLEAVED) {
      IFE_MHIP(m, hipMemcpyAsync(out + (size_t)(R.z0 * plane) * IFE_NUM_FEATURES, src,
                                 slab_vox * IFE_NUM_FEATURES * 4, hipMemcpyDeviceToHost, R.sd));
    } else {
      for (int c = 0; c < IFE_NUM_FEATURES; ++c)
        IFE_MHIP(m, hipMemcpyAsync(out + (size_t)c * (size_t)(nz * plane) + (size_t)(R.z0 * plane),
                                   src + (size_t)c * slab_vox, slab_vox * 4, hipMemcpyDeviceToHost, R.sd));
    }
  }
  return IFE_OK;
}

// Nothing of a call stays in flight behind its return and no event outlives it, whether the
// call succeeded or stopped half way (the copies read and write the caller's host buffers).
// `failed`: an error is already recorded in m->err and must stay the one reported.
int multi_drain(ife_multi *m, bool failed) {
  int result = IFE_OK;
  for (auto &R : m->ranks) {
    hipError_t e = hipSetDevice(R.dev);
    if (e == hipSuccess) e = hipStreamSynchronize(R.sc);
    if (e == hipSuccess) e = hipStreamSynchronize(R.sb);
    if (e == hipSuccess) e = hipStreamSynchronize(R.sd);
    if (e != hipSuccess && !failed && result == IFE_OK)
      result = mfail(m, IFE_E_HIP, "device %d: synchronisation failed: %s", R.dev, hipGetErrorString(e));
    for (auto ev : R.ev) (void)hipEventDestroy(ev);
    R.ev.clear();
    R.uploaded = nullptr;
  }
  (void)hipGetLastError();
  return result;
}

// The blocking calls: every scale of `path` enqueued, fetched and drained.
int multi_features(ife_multi *m, MultiPath path, const void *image, int image_dtype, const void *mask,
                   int mask_dtype, const ife_volume_desc *vol, const float *sigmas, int n_sigmas, float *out,
                   int layout) {
  if (!m) return IFE_E_ARG;
  if (m->streaming) return mfail(m, IFE_E_STATE, "a streaming call is in flight: ife_multi_emphysema_features_end first");
  int rc = out ? multi_run(m, path, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, layout)
               : mfail(m, IFE_E_ARG, "null pointer");
  const size_t vox8 = rc == IFE_OK ? (size_t)(vol->nx * vol->ny * vol->nz) * IFE_NUM_FEATURES : 0;
  for (int s = 0; s < n_sigmas && rc == IFE_OK; ++s) rc = multi_fetch_scale(m, s, out + (size_t)s * vox8);
  const int drained = multi_drain(m, rc != IFE_OK);
  return rc != IFE_OK ? rc : drained;
}

// The _begin calls: every scale of `path` enqueued; returns once the uploads have landed.
int multi_begin(ife_multi *m, MultiPath path, const void *image, int image_dtype, const void *mask,
                int mask_dtype, const ife_volume_desc *vol, const float *sigmas, int n_sigmas, int layout) {
  if (!m) return IFE_E_ARG;
  if (m->streaming) return mfail(m, IFE_E_STATE, "a streaming call is already in flight");
  int rc = multi_run(m, path, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, layout);
  for (auto &R : m->ranks) {  // the caller may reuse image and mask from here on
    if (rc != IFE_OK) break;
    hipError_t e = hipSetDevice(R.dev);
    if (e == hipSuccess && R.uploaded) e = hipEventSynchronize(R.uploaded);
    if (e != hipSuccess) rc = mfail(m, IFE_E_HIP, "device %d: upload: %s", R.dev, hipGetErrorString(e));
  }
  if (rc != IFE_OK) {
    (void)multi_drain(m, true);
    return rc;
  }
  m->streaming = true;
  return IFE_OK;
}

}  // namespace

extern "C" {

int ife_multi_emphysema_features(ife_multi *m, const void *image, int image_dtype, const void *mask,
                                 int mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                                 int n_sigmas, float *out, int layout) {
  return multi_features(m, MULTI_FD, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, out, layout);
}

// ife_differential_features over several devices: the same slabs and state chains, six Z jobs per
// scale, and behind them only slab-local work (multi_run, MULTI_JET).
int ife_multi_differential_features(ife_multi *m, const void *image, int image_dtype, const void *mask,
                                    int mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                                    int n_sigmas, float *out, int layout) {
  return multi_features(m, MULTI_JET, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, out, layout);
}

// The scale loop of tools/ExtractFeatures.cxx:132-154 over several devices, one scale at a time
// to the host: _begin uploads the slabs once, runs the prepass once and enqueues EVERY scale on
// every device (nothing is waited for); _fetch(k) blocks until scale k of every slab has been
// copied into `out` (the whole volume of that scale, host memory) while the later scales keep
// computing; _end drains.  The inputs may be reused once _begin returns: it waits for the uploads
// (from page-locked memory they run asynchronously to the host), not for the scales; `out` must
// stay valid until its _fetch returns.
int ife_multi_emphysema_features_begin(ife_multi *m, const void *image, int image_dtype, const void *mask,
                                       int mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                                       int n_sigmas, int layout) {
  return multi_begin(m, MULTI_FD, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, layout);
}

// The same stream with every scale that of ife_multi_differential_features; _fetch and _end are
// those of the stream above.
int ife_multi_differential_features_begin(ife_multi *m, const void *image, int image_dtype, const void *mask,
                                          int mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                                          int n_sigmas, int layout) {
  return multi_begin(m, MULTI_JET, image, image_dtype, mask, mask_dtype, vol, sigmas, n_sigmas, layout);
}

int ife_multi_emphysema_features_fetch(ife_multi *m, int scale, float *out) {
  if (!m) return IFE_E_ARG;
  if (!m->streaming) return mfail(m, IFE_E_STATE, "no streaming call in flight");
  if (scale < 0 || scale >= m->s_scales || !out) return mfail(m, IFE_E_ARG, "bad scale index or null output");
  int rc = multi_fetch_scale(m, scale, out);
  for (auto &R : m->ranks) {  // the copies of this scale have landed
    hipError_t e = hipSetDevice(R.dev);
    if (e == hipSuccess) e = hipStreamSynchronize(R.sd);
    if (e != hipSuccess && rc == IFE_OK) rc = mfail(m, IFE_E_HIP, "device %d: %s", R.dev, hipGetErrorString(e));
  }
  return rc;
}

int ife_multi_emphysema_features_end(ife_multi *m) {
  if (!m) return IFE_E_ARG;
  if (!m->streaming) return IFE_OK;
  m->streaming = false;
  return multi_drain(m, false);
}

}  // extern "C"
