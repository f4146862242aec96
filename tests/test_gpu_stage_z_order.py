"""The Z pass of a Z-slab with an order per job (ife_stage_z_sweep_order / _combine_order /
_fused_order): stitched over the slabs it is ife_stage_recursive_gaussian_order along z on the whole
volume bit for bit, for the orders 0, 1, 2, whichever of the two lean-sweep forms runs -- three
consecutive jobs of one source at the orders 0, 1, 2 take the shared-read kernel, every other job
order the per-job kernel -- and both forms leave the same bytes everywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIGMAS = (0.8, 2.5)
# (29, 5, 13): 65 lines = one full wave and one lane; slabs of 4 (the minimum), 13 (one register
# block of 12 plus one) and 12 planes (exactly one block).  (50, 20, 15): 300 lines = two line groups
# of 256, the second ragged; two slabs of 25 planes = three blocks, the last of one sample, two pairs.
CASES = {
    "small": dict(shape=(29, 5, 13), spacing=(1.0, 1.0, 1.25), bounds=[0, 4, 17, 29]),
    "wide": dict(shape=(50, 20, 15), spacing=(1.0, 1.0, 1.0), bounds=[0, 25, 50]),
}
ALL, SPLIT = "all", "split"


def line_groups(case, how):
    nz, ny, nx = CASES[case]["shape"]
    L = ny * nx
    return [(0, L)] if how == ALL else [(0, 256), (256, L - 256)]


def six_jobs(sigma, form):
    """(source, sigma, order) of the six Z jobs of one scale: source-major (the shared-read form
    applies to both sources) or interleaved (no three consecutive jobs share their input)."""
    if form == "major":
        return [(s, sigma, k) for s in range(2) for k in range(3)]
    return [(s, sigma, k) for k in range(3) for s in range(2)]


@pytest.fixture(scope="module")
def sources(synth):
    """Per case: the two float sources of the differential path, cT and c, on the host."""
    out = {}
    for name, c in CASES.items():
        img = synth.volume_f32(c["shape"], 17)
        cert = np.minimum(synth.mask_ellipsoids(c["shape"]), 1).astype(np.float32)
        cert[:, :2, :] = 1.0
        out[name] = [np.ascontiguousarray(img * cert), cert]
    return out


@pytest.fixture(scope="module")
def reference(ife, ctx, sources):
    """(case, source, sigma, order) -> the whole-volume pass along z, computed once and kept."""
    import torch
    cache = {}

    def get(case, src, sigma, order):
        key = (case, src, sigma, order)
        if key not in cache:
            c = CASES[case]
            vin = torch.from_numpy(sources[case][src]).cuda()
            vout = torch.empty_like(vin)
            ctx.stage_recursive_gaussian_order(vin.data_ptr(), vout.data_ptr(), c["shape"], c["spacing"], 2, sigma,
                                               order)
            torch.cuda.synchronize()
            cache[key] = vout.cpu().numpy()
            cache[key].setflags(write=False)
        return cache[key]
    return get


def run_slabs(ife, ctx, srcs, case, jobs, mode, groups, bounds=None, orders="given", old_api=False):
    """The Z pass of `jobs` over the slabs of the case.  mode "three": sweep, sweep, combine on
    every slab; "roles": the engine's rule (lower half lean causal sweep + anticausal fused, upper
    half the other way round).  Returns the stitched outputs per job and, per rank, the checkpoint
    areas per job and the outgoing states per (direction, line group)."""
    import torch
    c = CASES[case]
    bounds = bounds or c["bounds"]
    spacing = c["spacing"]
    W, nj = len(bounds) - 1, len(jobs)
    sig = [j[1] for j in jobs]
    ords = None if orders is None else [j[2] for j in jobs]
    ext, slabs = [], []
    for r in range(W):
        lo = ife.Z_OVERLAP_LO if r > 0 else 0
        hi = ife.Z_OVERLAP_HI if r < W - 1 else 0
        e = [torch.from_numpy(v[bounds[r] - lo:bounds[r + 1] + hi].copy()).cuda() for v in srcs]
        ext.append(e)
        slabs.append([t[lo:lo + bounds[r + 1] - bounds[r]] for t in e])   # views: data_ptr() is the slab's plane 0
    shp = [tuple(s[0].shape) for s in slabs]
    outs = [[torch.full(shp[r], float("nan"), dtype=torch.float32, device="cuda") for _ in range(nj)]
            for r in range(W)]
    cks = [[torch.zeros(ctx.stage_z_ck_bytes(shp[r]), dtype=torch.uint8, device="cuda") for _ in range(nj)]
           for r in range(W)]
    state = {(d, r, g): torch.zeros(nj * ife.Z_STATE_BYTES * nl, dtype=torch.uint8, device="cuda")
             for d in (0, 1) for r in range(W) for g, (l0, nl) in enumerate(groups)}

    def ins(r):
        return [slabs[r][j[0]].data_ptr() for j in jobs]

    def ck(r):
        return [t.data_ptr() for t in cks[r]]

    def sweep(r, d, g):
        l0, nl = groups[g]
        nb = r - 1 if d == 0 else r + 1
        has_nb = 0 <= nb < W
        sin = state[(d, nb, g)].data_ptr() if has_nb else None
        sout = state[(d, r, g)].data_ptr()
        if old_api:
            ctx.stage_z_sweep(d, ins(r), shp[r], spacing, l0, nl, sig, has_nb, sin, sout, ck(r))
        else:
            ctx.stage_z_sweep_order(d, ins(r), shp[r], spacing, l0, nl, sig, ords, has_nb, sin, sout, ck(r))

    def fused(r, d, g):
        l0, nl = groups[g]
        nb = r - 1 if d == 0 else r + 1
        sin = state[(d, nb, g)].data_ptr() if 0 <= nb < W else None
        o = [t.data_ptr() for t in outs[r]]
        if old_api:
            ctx.stage_z_fused(d, ins(r), o, shp[r], spacing, l0, nl, sig, r > 0, r < W - 1, sin,
                              state[(d, r, g)].data_ptr(), ck(r))
        else:
            ctx.stage_z_fused_order(d, ins(r), o, shp[r], spacing, l0, nl, sig, ords, r > 0, r < W - 1, sin,
                                    state[(d, r, g)].data_ptr(), ck(r))

    def combine(r, g):
        l0, nl = groups[g]
        o = [t.data_ptr() for t in outs[r]]
        if old_api:
            ctx.stage_z_combine(ins(r), o, shp[r], spacing, l0, nl, sig, r > 0, r < W - 1, ck(r))
        else:
            ctx.stage_z_combine_order(ins(r), o, shp[r], spacing, l0, nl, sig, ords, r > 0, r < W - 1, ck(r))

    for g in range(len(groups)):
        if mode == "three":
            for r in range(W):
                sweep(r, 0, g)
            for r in range(W - 1, -1, -1):
                sweep(r, 1, g)
            for r in range(W):
                combine(r, g)
        else:
            lean = [0 if r <= W - 1 - r else 1 for r in range(W)]
            for r in range(W):                      # the causal chain's lean part
                if lean[r] == 0:
                    sweep(r, 0, g)
            for r in range(W - 1, -1, -1):          # the anticausal chain's lean part
                if lean[r] == 1:
                    sweep(r, 1, g)
            for r in range(W):                      # causal carried on through the upper half
                if lean[r] == 1:
                    fused(r, 0, g)
            for r in range(W - 1, -1, -1):          # anticausal carried on through the lower half
                if lean[r] == 0:
                    fused(r, 1, g)
    torch.cuda.synchronize()
    return dict(
        out=[np.concatenate([outs[r][j].cpu().numpy() for r in range(W)], 0) for j in range(nj)],
        ck=[[t.cpu().numpy() for t in cks[r]] for r in range(W)],
        state={k: t.cpu().numpy().reshape(nj, -1) for k, t in state.items()})


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("form", ["major", "interleaved"])
@pytest.mark.parametrize("case,mode,how", [
    ("small", "three", ALL), ("small", "roles", ALL),
    ("wide", "three", ALL), ("wide", "three", SPLIT), ("wide", "roles", SPLIT)])
def test_stitched_slabs_equal_the_whole_volume(ife, ctx, sources, reference, case, mode, how, form, sigma):
    jobs = six_jobs(sigma, form)
    got = run_slabs(ife, ctx, sources[case], case, jobs, mode, line_groups(case, how))
    for j, (src, sg, order) in enumerate(jobs):
        want = reference(case, src, sg, order)
        assert np.array_equal(got["out"][j].view(np.uint32), want.view(np.uint32)), \
            "%s %s %s source %d sigma %g order %d" % (case, mode, form, src, sg, order)


@pytest.mark.parametrize("mode", ["three", "roles"])
@pytest.mark.parametrize("case,bounds,how", [
    ("small", None, ALL), ("small", [0, 29], ALL), ("wide", None, ALL), ("wide", None, SPLIT), ("wide", [0, 50], SPLIT)])
def test_shared_read_sweep_leaves_the_bytes_of_the_per_job_sweep(ife, ctx, sources, case, bounds, how, mode):
    """Slabs with no neighbour, one below, one above and both: outgoing states, checkpoint areas
    and outputs of the six jobs source-major (shared-read sweeps) against the same six interleaved
    (per-job sweeps)."""
    sigma = 2.5
    major, inter = six_jobs(sigma, "major"), six_jobs(sigma, "interleaved")
    groups = line_groups(case, how)
    a = run_slabs(ife, ctx, sources[case], case, major, mode, groups, bounds)
    b = run_slabs(ife, ctx, sources[case], case, inter, mode, groups, bounds)
    for ja, job in enumerate(major):
        jb = inter.index(job)
        assert np.array_equal(a["out"][ja].view(np.uint32), b["out"][jb].view(np.uint32)), ("out", job)
        assert not np.isnan(a["out"][ja]).any(), job
        for r in range(len(a["ck"])):
            assert np.array_equal(a["ck"][r][ja], b["ck"][r][jb]), ("checkpoints", r, job)
        for key in a["state"]:
            assert np.array_equal(a["state"][key][ja], b["state"][key][jb]), ("state", key, job)
    assert any(s.any() for s in a["state"].values()) and any(c.any() for c in a["ck"][0])


def test_both_forms_agree_under_the_line_options(ife, ctx, sources):
    """IFE_OPT_IIR_FMA selects the fused-multiply-add build of every slab kernel, the shared-read
    ones included, and IFE_OPT_IIR_BLOCK leaves the slab kernels alone, as on the existing calls."""
    major, inter = six_jobs(0.8, "major"), six_jobs(0.8, "interleaved")
    groups = line_groups("small", ALL)
    plain = run_slabs(ife, ctx, sources["small"], "small", major, "roles", groups)
    try:
        ctx.set_option(ife.OPT_IIR_BLOCK, 8)
        blocked = run_slabs(ife, ctx, sources["small"], "small", major, "roles", groups)
        ctx.set_option(ife.OPT_IIR_BLOCK, 0)
        ctx.set_option(ife.OPT_IIR_FMA, 1)
        a = run_slabs(ife, ctx, sources["small"], "small", major, "roles", groups)
        b = run_slabs(ife, ctx, sources["small"], "small", inter, "roles", groups)
    finally:
        ctx.set_option(ife.OPT_IIR_BLOCK, 0)
        ctx.set_option(ife.OPT_IIR_FMA, 0)
    for ja, job in enumerate(major):
        jb = inter.index(job)
        assert np.array_equal(blocked["out"][ja].view(np.uint32), plain["out"][ja].view(np.uint32)), job
        assert np.array_equal(a["out"][ja].view(np.uint32), b["out"][jb].view(np.uint32)), job
        for r in range(len(a["ck"])):
            assert np.array_equal(a["ck"][r][ja], b["ck"][r][jb]), ("checkpoints", r, job)
        for key in a["state"]:
            assert np.array_equal(a["state"][key][ja], b["state"][key][jb]), ("state", key, job)
        assert not np.isnan(a["out"][ja]).any(), job


@pytest.mark.parametrize("mode", ["three", "roles"])
def test_null_orders_are_the_existing_calls(ife, ctx, sources, reference, mode):
    jobs = [(0, 0.8, 0), (1, 0.8, 0), (0, 2.5, 0)]
    groups = line_groups("wide", SPLIT)
    new = run_slabs(ife, ctx, sources["wide"], "wide", jobs, mode, groups, orders=None)
    old = run_slabs(ife, ctx, sources["wide"], "wide", jobs, mode, groups, old_api=True)
    for j, (src, sg, order) in enumerate(jobs):
        assert np.array_equal(new["out"][j].view(np.uint32), old["out"][j].view(np.uint32))
        assert np.array_equal(new["out"][j].view(np.uint32), reference("wide", src, sg, 0).view(np.uint32))
        for r in range(len(new["ck"])):
            assert np.array_equal(new["ck"][r][j], old["ck"][r][j])
    for key in new["state"]:
        assert np.array_equal(new["state"][key], old["state"][key])


@pytest.mark.parametrize("bad", [3, -1])
def test_other_orders_are_refused(ife, ctx, bad):
    import torch
    shape, L = (8, 4, 16), 64
    vol = torch.zeros(shape, dtype=torch.float32, device="cuda")
    out = torch.zeros_like(vol)
    ck = torch.zeros(ctx.stage_z_ck_bytes(shape), dtype=torch.uint8, device="cuda")
    st = torch.zeros(ife.Z_STATE_BYTES * L, dtype=torch.uint8, device="cuda")
    one = (1.0, 1.0, 1.0)
    calls = [
        lambda: ctx.stage_z_sweep_order(0, [vol.data_ptr()], shape, one, 0, L, [1.0], [bad], False, None,
                                        st.data_ptr(), [ck.data_ptr()]),
        lambda: ctx.stage_z_combine_order([vol.data_ptr()], [out.data_ptr()], shape, one, 0, L, [1.0], [bad],
                                          False, False, [ck.data_ptr()]),
        lambda: ctx.stage_z_fused_order(1, [vol.data_ptr()], [out.data_ptr()], shape, one, 0, L, [1.0], [bad],
                                        False, False, None, st.data_ptr(), [ck.data_ptr()]),
    ]
    for call in calls:
        with pytest.raises(ife.IfeError) as e:
            call()
        assert e.value.code == ife.E_ARG
