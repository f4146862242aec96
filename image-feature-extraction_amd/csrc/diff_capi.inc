// diff_capi.inc -- the differential normalized convolution complete to second order
// (include/ife_hip.h: ife_normalized_convolution_jet, ife_differential_features, DESIGN.md
// section 4 "Differential features"); included at the end of ife_capi.hip (shares its context,
// staging, line-pass and profiling helpers), in front of scales_capi.inc, whose scale loop takes the
// twenty fields of a scale from here and hands them to its sinks.
//
// Pass tree.  For f in {cT, c} and every order triple (ox, oy, oz) with ox + oy + oz <= 2 the
// field F[ox,oy,oz](f) = RG_y^oy(RG_x^ox(RG_z^oz(f))) is built by line passes in ITK's order
// z, x, y, a float image between the passes:
//   z level   6 fields, one launch:    cT, c -> orders 0, 1, 2 (three jobs share one input)
//   x level  12 fields, two launches:  per source  z0 -> 0, 1, 2;  z1 -> 0, 1;  z2 -> 0
//   y level  20 fields, three launches (8 + 8 + 4 jobs): every x-level field of total order t
//            -> orders 0 .. 2 - t
// 38 field-passes per scale.  Then one pointwise kernel (feature_kernels.hpp: jet_kernel_*)
// turns the twenty fields into the jet or the features.
//
// Workspace.  The fields live in slots of one allocation of the call's own (ife_ctx::dj_ws).  A
// slot is taken when a launch writes a field and given back as soon as the last launch that reads
// the field has been enqueued (one stream: the next writer of the slot runs behind that reader),
// and the y launches are ordered so that the x-level fields with one consumer go first.  The peak
// is JET_SLOTS = 22 fields while the last y launch runs (the twenty results and its two inputs):
// 88 bytes per voxel.  Beside it: cT and c as float (8 bytes per voxel, ife_ctx::pre) and the
// checkpoints of eight concurrent line jobs (44 bytes per voxel): 140 bytes per voxel in all,
// plus the staging of image, mask and output in IFE_MEM_HOST mode.  Scales run one after the
// other over the same slots.  IFE_E_NOMEM when an allocation fails.

namespace {

constexpr int JET_SLOTS = 22;

// index of an order triple among the ten of the jet: 000, x, y, z, xx, xy, xz, yy, yz, zz
int jet_index(int ox, int oy, int oz) {
  static const int tab[3][3][3] = {  // [ox][oy][oz], -1 where ox + oy + oz > 2
      {{0, 3, 9}, {2, 8, -1}, {7, -1, -1}},
      {{1, 6, -1}, {5, -1, -1}, {-1, -1, -1}},
      {{4, -1, -1}, {-1, -1, -1}, {-1, -1, -1}}};
  return tab[ox][oy][oz];
}

// The slots of the workspace and who reads them still.
struct JetSlots {
  float *base;
  size_t pitch;  // floats per slot (a multiple of four: every slot starts on a 16-byte boundary)
  int readers[JET_SLOTS];
  bool used[JET_SLOTS];
  int take(int n_readers) {
    for (int s = 0; s < JET_SLOTS; ++s)
      if (!used[s]) { used[s] = true; readers[s] = n_readers; return s; }
    return -1;
  }
  void read_done(int s) {
    if (--readers[s] == 0) used[s] = false;
  }
  float *at(int s) const { return base + (size_t)s * pitch; }
};

// One launch of the tree: jobs (input slot or source, output slot, order) along one axis; the
// input slots are given back once the launch is enqueued.
struct JetLaunch {
  ife_ctx *ctx;
  const ife_volume_desc *vol;
  JetSlots *sl;
  double sigma;
  int axis, n = 0;
  const float *in[IIR_MAX_JOBS];
  float *out[IIR_MAX_JOBS];
  double sg[IIR_MAX_JOBS];
  int order[IIR_MAX_JOBS], in_slot[IIR_MAX_JOBS];
  JetLaunch(ife_ctx *c, const ife_volume_desc *v, JetSlots *s, double sig, int ax)
      : ctx(c), vol(v), sl(s), sigma(sig), axis(ax) {}
  // returns the output slot (-1: none left, which would be a mistake in the schedule)
  int add(const float *src, int src_slot, int ord, int out_readers) {
    const int o = sl->take(out_readers);
    if (o < 0 || n >= IIR_MAX_JOBS) return -1;
    in[n] = src_slot >= 0 ? sl->at(src_slot) : src;
    in_slot[n] = src_slot;
    out[n] = sl->at(o);
    sg[n] = sigma;
    order[n] = ord;
    ++n;
    return o;
  }
  int run() {
    const int rc = launch_iir(ctx, vol, axis, n, in, out, sg, 1, order);
    for (int j = 0; j < n; ++j)
      if (in_slot[j] >= 0) sl->read_done(in_slot[j]);
    return rc;
  }
};

// The Z-level fields of one scale: order k of source s (0 = cT, 1 = c), a slot of the workspace
// or (slot < 0) a field of the caller's (ife_stage_jet_features: the Z level of a Z-slab is made
// by the slab kernels).
struct JetZ {
  const float *p[2][3];
  int slot[2][3];
};

// The workspace of one scale for this volume, every slot free.
int jet_workspace(ife_ctx *ctx, const ife_volume_desc *vol, JetSlots *sl) {
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  sl->pitch = (n + 3) / 4 * 4;
  int rc = ensure(ctx, ctx->dj_ws, (size_t)JET_SLOTS * sl->pitch * sizeof(float));
  if (rc) return rc;
  sl->base = (float *)ctx->dj_ws.p;
  for (int s = 0; s < JET_SLOTS; ++s) { sl->used[s] = false; sl->readers[s] = 0; }
  return IFE_OK;
}

const char *const kJetBadSchedule = "the slot schedule of the differential convolution does not fit its workspace";

// The X and Y levels behind the Z level: the twenty fields of one scale from its six Z-level
// fields.  On return f points into the workspace; every other slot is free again.
int jet_fields_xy(ife_ctx *ctx, JetSlots &sl, const JetZ &z, const ife_volume_desc *vol, double sigma,
                  JetFields *f) {
  int rc;
  // x level, one launch per source: xs[s][ox][oz], read by 3 - ox - oz jobs of the y level
  int xs[2][3][3];
  for (int s = 0; s < 2; ++s) {
    JetLaunch L(ctx, vol, &sl, sigma, 0);
    for (int oz = 0; oz < 3; ++oz)
      for (int ox = 0; ox + oz < 3; ++ox)
        if ((xs[s][ox][oz] = L.add(z.p[s][oz], z.slot[s][oz], ox, 3 - ox - oz)) < 0)
          return fail(ctx, IFE_E_STATE, "%s", kJetBadSchedule);
    if ((rc = L.run())) return rc;
  }
  // y level: the jobs in the order that frees x-level fields soonest, cut into launches of eight
  struct YJob { int s, ox, oz, oy; };
  static const YJob yjobs[20] = {
      {0, 2, 0, 0}, {0, 1, 1, 0}, {0, 0, 2, 0}, {1, 2, 0, 0}, {1, 1, 1, 0}, {1, 0, 2, 0},  // one reader each
      {0, 1, 0, 0}, {0, 1, 0, 1},
      {1, 1, 0, 0}, {1, 1, 0, 1}, {0, 0, 1, 0}, {0, 0, 1, 1}, {1, 0, 1, 0}, {1, 0, 1, 1},
      {0, 0, 0, 0}, {0, 0, 0, 1},
      {0, 0, 0, 2}, {1, 0, 0, 0}, {1, 0, 0, 1}, {1, 0, 0, 2}};
  for (int j0 = 0; j0 < 20; j0 += IIR_MAX_JOBS) {
    JetLaunch L(ctx, vol, &sl, sigma, 1);
    for (int j = j0; j < std::min(20, j0 + IIR_MAX_JOBS); ++j) {
      const YJob &y = yjobs[j];
      const int o = L.add(nullptr, xs[y.s][y.ox][y.oz], y.oy, 1 << 20 /* the jet kernel: never given back */);
      if (o < 0) return fail(ctx, IFE_E_STATE, "%s", kJetBadSchedule);
      (y.s == 0 ? f->n : f->d)[jet_index(y.ox, y.oy, y.oz)] = sl.at(o);
    }
    if ((rc = L.run())) return rc;
  }
  return IFE_OK;
}

// The twenty fields of one scale from cT and c (device, float).  On return f points into the
// workspace; every other slot is free again.
int jet_fields(ife_ctx *ctx, const float *ct, const float *c, const ife_volume_desc *vol, double sigma,
               JetFields *f) {
  JetSlots sl;
  int rc = jet_workspace(ctx, vol, &sl);
  if (rc) return rc;
  const float *src[2] = {ct, c};
  // z level: order k of source s, read by 3 - k jobs of the x level
  JetZ z;
  JetLaunch L(ctx, vol, &sl, sigma, 2);
  for (int s = 0; s < 2; ++s)
    for (int k = 0; k < 3; ++k) {
      if ((z.slot[s][k] = L.add(src[s], -1, k, 3 - k)) < 0) return fail(ctx, IFE_E_STATE, "%s", kJetBadSchedule);
      z.p[s][k] = nullptr;
    }
  if ((rc = L.run())) return rc;
  return jet_fields_xy(ctx, sl, z, vol, sigma, f);
}

// What the pointwise kernels need of the volume (pvec is launch_jet's own).
JetGeom jet_geom(const ife_volume_desc *vol) {
  JetGeom g;
  g.nvox = vol->nx * vol->ny * vol->nz;
  const double sp[3] = {vol->sx, vol->sy, vol->sz};
  for (int a = 0; a < 3; ++a) g.r[a] = 1.0 / sp[a];
  int p = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) g.rr[p++] = g.r[i] * g.r[j];
  g.pvec = 0;
  return g;
}

// The pointwise pass over the twenty fields.  mask: FEATURES8 only (may be null).
template <int MODE, typename TM>
int launch_jet(ife_ctx *ctx, const JetFields &f, const TM *mask, float *out, const ife_volume_desc *vol,
               int layout) {
  const int64_t n = vol->nx * vol->ny * vol->nz;
  JetGeom g = jet_geom(vol);
  g.pvec = reinterpret_cast<uintptr_t>(out) % 16 == 0 && n % 4 == 0;
  // the fields are slots of the workspace (16-byte aligned); the mask decides the vector form
  const bool vec = reinterpret_cast<uintptr_t>(mask) % (4 * sizeof(TM)) == 0;
  const int64_t n4 = vec ? n / 4 : 0;
  const int planar = layout == IFE_PLANAR ? 1 : 0;
  ProfScope ps(ctx, KK_JET);
  auto launch = [&](auto TRIG, auto PL) {
    constexpr int T = decltype(TRIG)::value;
    constexpr bool P = decltype(PL)::value != 0;
    if (n4 > 0) {
      // grid-stride over the pieces: at most eight workgroups per CU's worth of blocks
      const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 256 * 8);
      hipLaunchKernelGGL((jet_kernel_vec4<MODE, T, P, TM>), dim3(blocks), dim3(256), 0, ctx->stream, f, mask, out, g,
                         n4);
    }
    if (n4 * 4 < n) {
      const unsigned blocks = (unsigned)std::min<int64_t>((n - n4 * 4 + 255) / 256, 256 * 8);
      hipLaunchKernelGGL((jet_kernel_scalar<MODE, T, P, TM>), dim3(blocks), dim3(256), 0, ctx->stream, f, mask, out,
                         g, n4 * 4, n);
    }
  };
  with_const<1, 0>(planar, [&](auto PL) {
    if constexpr (MODE == JET_FEATURES8) with_const<1, 2, 0>(ctx->trig_mode, [&](auto TRIG) { launch(TRIG, PL); });
    else launch(std::integral_constant<int, 0>{}, PL);
  });
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

// IFE_OPT_DIFFERENTIAL: the features of the sampled voxels of one scale straight from the twenty
// fields into eight sample columns (stats_capi.inc); one wave per 64-voxel row segment.  They share
// the jet's row of the kernel-time table.
int launch_jet_samples(ife_ctx *ctx, const JetFields &f, const ife_volume_desc *vol, const JetSampleSink &sk) {
  const JetGeom g = jet_geom(vol);
  ProfScope ps(ctx, KK_JET);
  const unsigned blocks = (unsigned)((sk.nseg + 3) / 4);  // nseg < 2^31 (the caller's check)
  with_const<1, 2, 0>(ctx->trig_mode, [&](auto TRIG) {
    hipLaunchKernelGGL((jet_samples_kernel<decltype(TRIG)::value>), dim3(blocks), dim3(256), 0, ctx->stream, f, g, sk);
  });
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

// IFE_OPT_DIFFERENTIAL: the eight planes of bin codes of one scale straight from the twenty fields
// (dense_capi.inc).  mask: the clamped labels.  The 4-byte form where mask, codes and the plane
// stride allow it, the scalar form for the rest.
int launch_jet_codes(ife_ctx *ctx, const JetFields &f, const uint8_t *mask, const ife_volume_desc *vol,
                     const JetCodeSink &ck) {
  const JetGeom g = jet_geom(vol);
  const int64_t n = g.nvox;
  const bool vec = reinterpret_cast<uintptr_t>(mask) % 4 == 0 && reinterpret_cast<uintptr_t>(ck.code) % 4 == 0 &&
                   ck.stride % 4 == 0;
  const int64_t n4 = vec ? n / 4 : 0;
  ProfScope ps(ctx, KK_JET);
  with_const<1, 2, 0>(ctx->trig_mode, [&](auto TRIG) {
    constexpr int T = decltype(TRIG)::value;
    if (n4 > 0)
      hipLaunchKernelGGL((jet_codes_kernel_vec4<T>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, ctx->stream, f,
                         mask, g, ck, n4);
    if (n4 * 4 < n)
      hipLaunchKernelGGL((jet_codes_kernel_scalar<T>), dim3((unsigned)((n - n4 * 4 + 255) / 256)), dim3(256), 0,
                         ctx->stream, f, mask, g, ck, n4 * 4, n);
  });
  IFE_HIP(ctx, hipGetLastError());
  return IFE_OK;
}

// cT = float(image) * float(mask) and c = float(mask) into ife_ctx::pre (c = 1 without a mask)
template <typename TI, typename TM>
int jet_sources(ife_ctx *ctx, const TI *img, const TM *msk, int64_t n) {
  const size_t nb = (size_t)((n + 3) / 4 * 4) * sizeof(float);
  int rc = ensure(ctx, ctx->pre[0], nb);
  if (!rc) rc = ensure(ctx, ctx->pre[1], nb);
  if (rc) return rc;
  float *tc = (float *)ctx->pre[0].p, *cf = (float *)ctx->pre[1].p;
  if ((rc = launch_prep<TI, TM>(ctx, img, msk, tc, cf, n))) return rc;
  if (msk == nullptr) {
    ProfScope ps(ctx, KK_PREP);
    const int64_t n4 = (int64_t)(nb / 16);
    const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 0x7fffffff);
    hipLaunchKernelGGL(stream_fill_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (float4 *)cf, n4, 1.0f);
    IFE_HIP(ctx, hipGetLastError());
  }
  return IFE_OK;
}

}  // namespace

extern "C" {

int ife_normalized_convolution_jet(ife_ctx *ctx, const float *image, const float *certainty,
                                   const ife_volume_desc *vol, double sigma, float *out10, int layout, int mem) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, vol, true))) return rc;
  if ((rc = check_layout_mem(ctx, layout, mem))) return rc;
  if (!image || !certainty || !out10) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_sigma(ctx, sigma))) return rc;
  const size_t n = (size_t)(vol->nx * vol->ny * vol->nz);
  const void *dI, *dC;
  void *dO;
  if ((rc = stage_in(ctx, mem, image, n * 4, ctx->st_img, &dI))) return rc;
  if ((rc = stage_in(ctx, mem, certainty, n * 4, ctx->st_aux, &dC))) return rc;
  if ((rc = stage_out_begin(ctx, mem, out10, n * 40, &dO))) return rc;
  if ((rc = check_in_alignment(ctx, dI, 4, dC, 4))) return rc;
  if ((rc = check_out_alignment(ctx, dO, 10, layout))) return rc;
  if ((rc = ensure(ctx, ctx->pre[0], (n + 3) / 4 * 4 * sizeof(float)))) return rc;
  float *tc = (float *)ctx->pre[0].p;
  if ((rc = launch_prep<float, float>(ctx, (const float *)dI, (const float *)dC, tc, nullptr, (int64_t)n)))
    return rc;
  JetFields f;
  if ((rc = jet_fields(ctx, tc, (const float *)dC, vol, sigma, &f))) return rc;
  if ((rc = launch_jet<JET_JET10>(ctx, f, (const uint8_t *)nullptr, (float *)dO, vol, layout))) return rc;
  return stage_out_end(ctx, mem, out10, n * 40);
}


int ife_stage_jet_features(ife_ctx *ctx, const float *const zf[6], const void *mask, int mask_dtype,
                           const ife_volume_desc *slab, double sigma, float *out, int layout) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = check_vol(ctx, slab, false))) return rc;
  if ((rc = check_layout_mem(ctx, layout, IFE_MEM_DEVICE))) return rc;
  if (!zf || !out) return fail(ctx, IFE_E_ARG, "null pointer");
  if ((rc = check_mask_dtype(ctx, mask, mask_dtype, true))) return rc;
  if ((rc = check_sigma(ctx, sigma))) return rc;
  if ((rc = check_axis_len(ctx, slab, 0)) || (rc = check_axis_len(ctx, slab, 1))) return rc;
  if ((rc = check_in_alignment(ctx, mask, mask && mask_dtype == IFE_U16 ? 2 : 1, nullptr, 1))) return rc;
  if ((rc = check_out_alignment(ctx, out, IFE_NUM_FEATURES, layout))) return rc;
  JetZ z;
  for (int s = 0; s < 2; ++s)
    for (int k = 0; k < 3; ++k) {
      if (!zf[3 * s + k]) return fail(ctx, IFE_E_ARG, "null pointer");
      z.p[s][k] = zf[3 * s + k];
      z.slot[s][k] = -1;
    }
  JetSlots sl;
  if ((rc = jet_workspace(ctx, slab, &sl))) return rc;
  JetFields f;
  if ((rc = jet_fields_xy(ctx, sl, z, slab, sigma, &f))) return rc;
  return with_mask_type(mask != nullptr, mask_dtype, mask, [&](auto msk) {
    return launch_jet<JET_FEATURES8>(ctx, f, msk, out, slab, layout);
  });
}

}  // extern "C"
