"""GPU parity tests: the HIP path, called through the C-ABI, against the CPU oracle on
the same seeded inputs.

Tolerances
  * everything up to and including the Hessian is IEEE add/mul/div/sqrt on identical
    operands in identical order (both sides built with -ffp-contract=off), so the bar
    is BIT-EXACT (compared as floats, i.e. -0.0 == +0.0).
  * eigenvalues / derived scalars: north_star bar is 1e-5 relative; measured against
    max(|lambda_1|, tiny) per voxel because the trigonometric solver's error is absolute
    in ||A||.  With IFE_OPT_TRIG_MODE=0 the device evaluates acos/cos in double like
    the oracle, so in practice these agree to <= 1 float ulp; the test asserts 1e-6
    (ten times tighter than the bar) and reports the exact-match fraction.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REL_TOL = 1e-6  # asserted; north_star allows 1e-5


def eig_rel_err(got, ref):
    """max |got-ref| / max(|ref lambda_1|, tiny) over voxels; arrays (..., >=3)."""
    scale = np.maximum(np.abs(ref[..., 0:1]).astype(np.float64), 1e-30)
    return float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / scale).max())


def assert_features_close(got, ref, mask=None):
    """got/ref: (..., 8) [S, G, e1, e2, e3, LoG, prod, frob] or (..., 6) eigen features."""
    nc = got.shape[-1]
    assert got.shape == ref.shape
    assert np.isfinite(got).all() == np.isfinite(ref).all()
    e0 = nc - 6
    if nc == 8:
        np.testing.assert_array_equal(got[..., 0], ref[..., 0])  # smoothed value
        np.testing.assert_array_equal(got[..., 1], ref[..., 1])  # gradient magnitude
    g, r = got[..., e0:], ref[..., e0:]
    lam = np.maximum(np.abs(r[..., 0]).astype(np.float64), 1e-30)
    d = np.abs(g.astype(np.float64) - r.astype(np.float64))
    assert (d[..., 0:4] / lam[..., None]).max() <= REL_TOL      # e1, e2, e3, LoG
    assert (d[..., 4] / lam ** 3).max() <= 3 * REL_TOL          # product
    assert (d[..., 5] / lam).max() <= REL_TOL                   # Frobenius
    if mask is not None:
        assert (got[mask == 0] == 0).all()


# ---------------------------------------------------------------------------------
# a1 / a2
# ---------------------------------------------------------------------------------
def _eigen_cases(rng):
    kat = json.load(open(os.path.join(HERE, "golden", "eigen_kat.json")))["cases"]
    mats = [c["A"] for c in kat]
    # diagonal branch: all orderings, magnitude ties, sign ties, zeros
    for d in ([3, 2, 1], [1, 3, 2], [2, 1, 3], [1, 2, 3], [3, 1, 2], [2, 3, 1], [1, 1, 1],
              [1, -1, 0], [-1, 1, 0], [2, 2, 1], [1, 2, 2], [2, 1, 2], [0, 0, 0], [-2, 2, -2],
              [0, 0, 5], [5, 0, 0], [0, -5, 0]):
        mats.append([d[0], 0, 0, d[1], 0, d[2]])
    # two equal eigenvalues (r = +-1 clamps), near-degenerate
    mats += [[2, 1, 1, 2, 1, 2], [-2, 1, 1, -2, 1, -2], [1, 1e-4, 0, 1, 0, 1], [1, 0, 0, 1, 1e-7, 1],
             [5, 0, 0, 5, 0, -1], [1, 1, 0, 1, 0, 3]]
    mats = np.array(mats, np.float32)
    rnd = []
    for dec in range(-6, 7, 2):
        rnd.append((rng.standard_normal((600, 6)) * 10.0 ** dec).astype(np.float32))
    # tiny off-diagonals that underflow p to 0 in float
    t = rng.standard_normal((200, 6)).astype(np.float32)
    t[:, [1, 2, 4]] *= np.float32(1e-30)
    rnd.append(t)
    return np.concatenate([mats] + rnd, 0)


@pytest.mark.parametrize("trig", [0, 1])
def test_eigen_batch_matches_oracle(ctx, ife, oracle, trig):
    A = _eigen_cases(np.random.default_rng(7))
    ctx.set_option(ife.OPT_TRIG_MODE, trig)
    try:
        ev = ctx.eigenvalues(A)
        ft = ctx.eigenvalue_features(A)
    finally:
        ctx.set_option(ife.OPT_TRIG_MODE, 0)
    ev_ref = oracle.eig3(A, trig)
    ft_ref = oracle.eigfeat(A, trig)
    assert eig_rel_err(ev, ev_ref) <= REL_TOL
    assert_features_close(ft, ft_ref)
    # ordering contract: |e0| >= |e1| >= |e2|
    a = np.abs(ev)
    assert (a[:, 0] >= a[:, 1]).all() and (a[:, 1] >= a[:, 2]).all()
    # the diagonal branch is pure selection: bit exact
    diag = (A[:, 1] == 0) & (A[:, 2] == 0) & (A[:, 4] == 0)
    np.testing.assert_array_equal(ev[diag], ev_ref[diag])
    exact = float((ev == ev_ref).mean())
    print("trig=%d eigenvalues bit-identical fraction: %.6f" % (trig, exact))
    if trig == 0:
        assert exact > 0.999


def test_eigen_kat_on_device(ctx):
    """The reference's own known answers, through the float solver on the GPU."""
    kat = json.load(open(os.path.join(HERE, "golden", "eigen_kat.json")))["cases"]
    A = np.array([c["A"] for c in kat], np.float32)
    ev = ctx.eigenvalues(A)
    for c, got in zip(kat, ev):
        exp = np.array(c["expected"], np.float64)
        tol = 2e-6 * max(1.0, np.abs(exp).max())  # float32 solver vs double expectations
        assert np.abs(got - exp).max() <= tol, (c["name"], got, exp)


def test_eigen_nan_propagates(ctx):
    A = np.array([[np.nan, 1, 0, 1, 0, 1], [1, np.nan, 0, 1, 0, 1]], np.float32)
    ev = ctx.eigenvalues(A)
    assert np.isnan(ev[1]).all()
    assert np.isnan(ev[0]).any()


# ---------------------------------------------------------------------------------
# a4: recursive Gaussian / normalized convolution  (bit exact)
# ---------------------------------------------------------------------------------
SHAPES = [(33, 36, 40), (4, 4, 4), (5, 70, 9), (17, 8, 129), (64, 64, 64)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma,spacing", [(1.0, (1, 1, 1)), (2.5, (0.7, 0.8, 1.25)),
                                           (0.6, (1, 1, 1))])
def test_normalized_convolution_bit_exact(ctx, oracle, synth, shape, sigma, spacing):
    img = synth.volume_f32(shape, 1234)
    cert = (synth.mask_ellipsoids(shape) > 0).astype(np.float32)
    cert[0, 0, 0] = 1.0
    cert += np.float32(0.25) * (np.arange(cert.size).reshape(shape) % 3 == 0)  # fractional weights
    got = ctx.normalized_gaussian_convolution(img, cert, sigma, spacing)
    ref = oracle.normalized_gaussian_convolution(img, cert, sigma, spacing)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("block", [8, 10, 12, 16])
def test_iir_block_size_is_invisible(ctx, ife, oracle, synth, block):
    shape = (37, 41, 45)
    img = synth.volume_f32(shape, 99)
    cert = np.ones(shape, np.float32)
    ctx.set_option(ife.OPT_IIR_BLOCK, block)
    try:
        got = ctx.normalized_gaussian_convolution(img, cert, 3.0)
    finally:
        ctx.set_option(ife.OPT_IIR_BLOCK, 0)  # the default
    np.testing.assert_array_equal(got, oracle.normalized_gaussian_convolution(img, cert, 3.0))


@pytest.mark.parametrize("shape,sigma,spacing", [((33, 36, 40), 1.5, (1, 1, 1)),
                                                 ((17, 8, 129), 2.5, (0.7, 0.8, 1.25)),
                                                 ((4, 5, 70), 0.8, (1, 1, 1))])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_differential_normalized_convolution_bit_exact(ctx, oracle, synth, shape, sigma, spacing, axis):
    """Row f4: ITK's first-order recursive Gaussian along `axis` inside the normalized
    convolution, on the line kernels; same bits as the oracle's restatement."""
    img = synth.volume_f32(shape, 77)
    cert = (synth.mask_ellipsoids(shape) > 0).astype(np.float32)
    cert[0, 0, 0] = 1.0
    cert += np.float32(0.25) * (np.arange(cert.size).reshape(shape) % 3 == 0)
    got = ctx.differential_normalized_convolution(img, cert, sigma, axis, spacing)
    ref = oracle.differential_normalized_convolution(img, cert, sigma, axis, spacing)
    np.testing.assert_array_equal(got, ref)


def test_zero_certainty_gives_flt_max(ctx, oracle):
    shape = (12, 12, 12)
    img = np.ones(shape, np.float32)
    cert = np.zeros(shape, np.float32)
    got = ctx.normalized_gaussian_convolution(img, cert, 1.0)
    assert (got == np.finfo(np.float32).max).all()
    np.testing.assert_array_equal(got, oracle.normalized_gaussian_convolution(img, cert, 1.0))


# ---------------------------------------------------------------------------------
# a3 / gradient magnitude (bit exact)
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 10, 70), (33, 36, 40), (1, 5, 7), (3, 1, 130), (70, 9, 3)])
@pytest.mark.parametrize("spacing", [(1, 1, 1), (0.7, 0.8, 1.25)])
def test_hessian3d_and_gradient_bit_exact(ctx, ife, oracle, synth, shape, spacing):
    img = synth.volume_f32(shape, 5)
    h = ctx.hessian3d(img, spacing)
    np.testing.assert_array_equal(h, oracle.hessian3d(img, spacing))
    hp = ctx.hessian3d(img, spacing, layout=ife.PLANAR)
    np.testing.assert_array_equal(np.moveaxis(hp, 0, -1), h)
    g = ctx.gradient_magnitude(img, spacing)
    np.testing.assert_array_equal(g, oracle.gradient_magnitude(img, spacing))


def test_hessian_spacing_power_option(ctx, ife, oracle, synth):
    shape = (12, 13, 14)
    img = synth.volume_f32(shape, 6)
    sp = (0.5, 2.0, 1.5)
    ctx.set_option(ife.OPT_DSCALE_MODE, 1)
    try:
        h = ctx.hessian3d(img, sp)
    finally:
        ctx.set_option(ife.OPT_DSCALE_MODE, 0)
    np.testing.assert_array_equal(h, oracle.hessian3d(img, sp, dscale=oracle.DSCALE_POW))


# ---------------------------------------------------------------------------------
# a5: the full per-scale feature vector
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sigmas,spacing", [
    ((33, 36, 40), [1.0, 2.0], (1, 1, 1)),
    ((64, 64, 64), [1.0, 2.0, 4.0], (1, 1, 1)),
    ((20, 70, 130), [1.5], (0.7, 0.7, 1.0)),
    ((4, 4, 4), [1.0], (1, 1, 1)),
])
def test_emphysema_features_match_oracle(ctx, ife, oracle, synth, shape, sigmas, spacing):
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)  # clamp as the tools do
    mask[0, 0, :] = 1
    got = ctx.emphysema_features(img, mask, sigmas, spacing)
    assert got.shape == (len(sigmas),) + shape + (8,)
    for s, sigma in enumerate(sigmas):
        ref = oracle.emphysema_features(img, mask, sigma, spacing)
        assert_features_close(got[s], ref, mask)
        print("sigma %.1f: all-8-components bit-identical fraction %.6f"
              % (sigma, float((got[s] == ref).mean())))
    planar = ctx.emphysema_features(img, mask, sigmas, spacing, layout=ife.PLANAR)
    np.testing.assert_array_equal(np.moveaxis(planar, 1, -1), got)


def test_emphysema_int16_image_u16_mask_labels(ctx, oracle, synth):
    """int16 CT-like input and an unclamped label mask (0/1/2): the mask VALUE is the
    certainty weight (ImageToEmphysemaFeaturesFilter.hxx:25), zero test for masking."""
    shape = (30, 34, 38)
    img = synth.volume_i16(shape, synth.SEED_CONFIG[5])
    labels = synth.mask_ellipsoids(shape)
    got = ctx.emphysema_features(img, labels.astype(np.uint16), [1.5], (0.7, 0.7, 1.0))[0]
    ref = oracle.emphysema_features(img.astype(np.float32), labels, 1.5, (0.7, 0.7, 1.0))
    assert_features_close(got, ref, labels)


def test_emphysema_stream_equals_one_call(ctx, ife, synth):
    """begin / fetch / end (upload and prepass once, scale by scale to the host) returns the
    volumes of the one-call form; fetching a scale that was not started is a state error."""
    shape = (24, 28, 32)
    img = synth.volume_i16(shape, 13)
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint16)
    sig = [1.0, 2.0, 3.0, 4.0]  # more scales than run through the line kernels at once
    whole = ctx.emphysema_features(img, mask, sig, (0.7, 0.7, 1.0))
    for k, vol in enumerate(ctx.emphysema_features_stream(img, mask, sig, (0.7, 0.7, 1.0))):
        np.testing.assert_array_equal(vol, whole[k])
    out = np.empty(shape + (8,), np.float32)
    rc = ctx._lib.ife_emphysema_features_fetch(ctx._h, 0, out.ctypes.data)
    assert rc == ife.E_STATE


def _page_locked(a):
    """A numpy view of a page-locked (pinned) copy of `a`: the uploads from it run
    asynchronously to the host."""
    import torch
    t = torch.from_numpy(a.view({2: np.int16, 4: np.float32, 1: np.uint8}[a.itemsize])).pin_memory()
    assert t.is_pinned()
    return t, t.numpy().view(a.dtype)


def _overwrite_back_to_front(dst, src):
    """The planes last in the upload order first, so that a copy still in flight would read them."""
    for z in range(dst.shape[0] - 1, -1, -1):
        dst[z] = src[z]


def test_emphysema_begin_inputs_reusable_once_it_returns(ife, synth):
    """ife_emphysema_features_begin from page-locked memory, image and mask overwritten with
    another volume as soon as it returns (mask first: it is uploaded last), every scale
    fetched: bit-identical to the blocking call on the original volume.  _begin must not
    return before its uploads have landed (include/ife_hip.h)."""
    import ctypes as C
    shape, spacing, sig = (128, 384, 384), (1.0, 1.0, 1.0), [1.0, 2.0]
    img = synth.volume_f32(shape, 23)
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    with ife.Context(0) as c:
        c.set_option(ife.OPT_TRIG_MODE, 0)
        want = c.emphysema_features(img, mask, sig, spacing)
        keep_i, p_img = _page_locked(img)
        keep_m, p_mask = _page_locked(mask)
        other_img = synth.volume_f32(shape, 24)
        other_mask = (synth.volume_f32(shape, 25) > 300).astype(np.uint8)
        d = ife._desc(shape, spacing)
        sigs = (C.c_float * len(sig))(*sig)
        rc = c._lib.ife_emphysema_features_begin(c._h, p_img.ctypes.data, ife.F32, p_mask.ctypes.data, ife.U8,
                                                  C.byref(d), sigs, len(sig), ife.INTERLEAVED)
        assert rc == ife.OK, c._lib.ife_last_error(c._h)
        _overwrite_back_to_front(p_mask, other_mask)
        _overwrite_back_to_front(p_img, other_img)
        try:
            for k in range(len(sig)):
                out = np.empty(shape + (8,), np.float32)
                assert c._lib.ife_emphysema_features_fetch(c._h, k, out.ctypes.data) == ife.OK
                assert np.array_equal(out.view(np.uint32), want[k].view(np.uint32)), \
                    "scale %d differs: _begin returned before its uploads had landed" % k
        finally:
            assert c._lib.ife_emphysema_features_end(c._h) == ife.OK


def test_emphysema_null_mask_equals_ones_mask(ctx, synth):
    shape = (24, 28, 32)
    img = synth.volume_f32(shape, 11)
    a = ctx.emphysema_features(img, None, [2.0])
    b = ctx.emphysema_features(img, np.ones(shape, np.uint8), [2.0])
    np.testing.assert_array_equal(a, b)


def test_normalized_convolution_where_the_certainty_vanishes(ctx, oracle, synth):
    """Half of the volume without certainty: far from the support the smoothed denominator
    is tiny (1e-30 and below) but not zero, so the quotient of two tiny numbers must come out
    exactly as the oracle's."""
    shape = (9, 70, 66)
    img = synth.volume_f32(shape, 21)
    cert = (synth.mask_ellipsoids(shape) > 0).astype(np.float32)
    cert[:, : shape[1] // 2, :] = 0.0
    cert += np.float32(0.25) * (np.arange(cert.size).reshape(shape) % 3 == 0) * (cert > 0)
    got = ctx.normalized_gaussian_convolution(img, cert, 0.7)
    ref = oracle.normalized_gaussian_convolution(img, cert, 0.7)
    np.testing.assert_array_equal(got, ref)
    assert np.abs(ref[cert == 0]).max() < np.finfo(np.float32).max  # tiny denominators, finite quotients


@pytest.mark.parametrize("block", [0, 8, 16])
@pytest.mark.parametrize("shape", [(24, 28, 32), (9, 70, 66), (5, 4, 130), (6, 25, 200)])
def test_fused_divide_option_is_invisible(ctx, ife, oracle, synth, shape, block):
    """The last axis pass stores numerator / denominator (IFE_OPT_FUSED_DIVIDE=1, default:
    sibling waves exchange through LDS) or two fields that the feature kernel divides (=0):
    same bits, both equal to the oracle -- ragged line counts, partial blocks, fractional
    certainties and the a4 entry point included."""
    img = synth.volume_f32(shape, 21)
    labels = synth.mask_ellipsoids(shape).astype(np.uint8)
    labels[0, 0, :] = 2
    ctx.set_option(ife.OPT_IIR_BLOCK, block)
    try:
        a = ctx.emphysema_features(img, labels, [1.0, 2.5])
        cert = (labels > 0).astype(np.float32)
        cert += np.float32(0.25) * (np.arange(cert.size).reshape(shape) % 3 == 0)
        na = ctx.normalized_gaussian_convolution(img, cert, 0.9)
        ctx.set_option(ife.OPT_FUSED_DIVIDE, 0)
        b = ctx.emphysema_features(img, labels, [1.0, 2.5])
        nb = ctx.normalized_gaussian_convolution(img, cert, 0.9)
    finally:
        ctx.set_option(ife.OPT_FUSED_DIVIDE, 1)
        ctx.set_option(ife.OPT_IIR_BLOCK, 0)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(na, nb)
    np.testing.assert_array_equal(na, oracle.normalized_gaussian_convolution(img, cert, 0.9))
    for s, sigma in enumerate((1.0, 2.5)):
        assert_features_close(a[s], oracle.emphysema_features(img, labels, sigma), labels)


@pytest.mark.parametrize("shape,kind", [((40, 70, 130), "exterior"), ((24, 28, 200), "ones"),
                                        ((9, 140, 66), "slabs"), ((5, 4, 6), "tiny")])
def test_constant_line_shortcut_is_invisible(ctx, ife, oracle, synth, shape, kind):
    """IFE_OPT_CONST_LINES=1 (default) copies lines that are all 0 -- or all 1 where the host
    found the filter to keep them -- instead of filtering them; =0 filters every line.  Same
    bits, and both equal to the oracle: masks with a large exterior (whole waves of zero
    lines along every axis), an all-ones mask (denominator lines of ones), masks made of
    slabs (constant along one axis only), exact zeros inside the image."""
    img = synth.volume_f32(shape, 33)
    nz, ny, nx = shape
    if kind == "exterior":
        mask = np.zeros(shape, np.uint8)
        mask[10:30, 20:50, 30:100] = 1
    elif kind == "ones":
        mask = np.ones(shape, np.uint8)
        img[:, :, :70] = 0.0                      # numerator lines of zeros along x only in part
        img[:, :10, :] = 0.0
    elif kind == "slabs":
        mask = np.zeros(shape, np.uint8)
        mask[:, 64:, :] = 1                       # constant along z and x, a step along y
        img[:, 70:, :] = 1.0                      # numerator lines of ones
    else:
        mask = np.ones(shape, np.uint8)
    sig = [1.0, 3.0]
    a = ctx.emphysema_features(img, mask, sig)
    nc_a = ctx.normalized_gaussian_convolution(img, mask.astype(np.float32), 2.0)
    ctx.set_option(ife.OPT_CONST_LINES, 0)
    try:
        b = ctx.emphysema_features(img, mask, sig)
        nc_b = ctx.normalized_gaussian_convolution(img, mask.astype(np.float32), 2.0)
    finally:
        ctx.set_option(ife.OPT_CONST_LINES, 1)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(nc_a, nc_b)
    np.testing.assert_array_equal(nc_a, oracle.normalized_gaussian_convolution(img, mask.astype(np.float32), 2.0))
    for s, sigma in enumerate(sig):
        ref = oracle.emphysema_features(img, mask, sigma)
        # far inside a region of exact zeros the smoothed field decays to ~1e-24 and the
        # reference's float p underflows: 0/0 in its solver, NaN in the same voxels here
        nan = np.isnan(ref)
        np.testing.assert_array_equal(np.isnan(a[s]), nan)
        assert_features_close(np.where(nan, 0, a[s]), np.where(nan, 0, ref), mask)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_constant_line_shortcut_keeps_the_sign_of_zero(ctx, ife, oracle, axis):
    """Lines of +0, of -0 (T * 0 where T < 0: the exterior of a CT numerator), of mixed zeros,
    of ones and of another constant, on every axis: with the shortcut on, the output has the
    bit patterns -- signs of zero included -- of the filtered line (shortcut off, and the
    oracle)."""
    import torch
    shape = (70, 130, 72)                                   # z, y, x: partial waves on every axis
    rng = np.random.default_rng(5)
    vol = rng.standard_normal(shape).astype(np.float32)
    mv = np.moveaxis(vol, 2 - axis, 0)                      # lines of this axis first: [n][a][b]
    na, nb = mv.shape[1], mv.shape[2]
    kind = (np.arange(na)[:, None] // 3 + np.arange(nb)[None, :] // 70) % 7
    mv[:, kind == 0] = 0.0
    mv[:, kind == 1] = -0.0
    mv[:, kind == 2] = 1.0
    mv[:, kind == 3] = 2.5
    alt = np.where(np.arange(mv.shape[0]) % 2 == 0, 0.0, -0.0).astype(np.float32)
    mv[:, kind == 4] = alt[:, None]                         # zeros of both signs along the line
    assert np.signbit(vol).any() and (vol == 0).any()
    d_in = torch.from_numpy(np.ascontiguousarray(vol)).cuda()
    res = {}
    for opt in (1, 0):
        ctx.set_option(ife.OPT_CONST_LINES, opt)
        try:
            for sigma in (1.0, 2.7):
                d_out = torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
                ctx.stage_recursive_gaussian(d_in.data_ptr(), d_out.data_ptr(), shape, (1.0, 1.0, 1.0),
                                             axis, sigma)
                ctx.synchronize()
                res[opt, sigma] = d_out.cpu().numpy()
        finally:
            ctx.set_option(ife.OPT_CONST_LINES, 1)
    for sigma in (1.0, 2.7):
        ref = oracle.recursive_gaussian_axis(vol, axis, sigma)
        for opt in (1, 0):
            np.testing.assert_array_equal(res[opt, sigma].view(np.uint32), ref.view(np.uint32),
                                          err_msg="axis %d sigma %g const_lines %d" % (axis, sigma, opt))


def test_emphysema_chunking_is_invisible(ctx, ife, synth):
    shape = (50, 20, 70)
    img = synth.volume_f32(shape, 12)
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    base = ctx.emphysema_features(img, mask, [1.0])
    for zc in (1, 7, 50, 1000):
        ctx.set_option(ife.OPT_ZCHUNK, zc)
        try:
            np.testing.assert_array_equal(ctx.emphysema_features(img, mask, [1.0]), base)
        finally:
            ctx.set_option(ife.OPT_ZCHUNK, 64)


# ---------------------------------------------------------------------------------
# a6 / a7 / a8 tool bodies
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64, 64), (21, 9, 67)])
def test_fd_hessian_features(ctx, ife, oracle, synth, shape):
    img = synth.volume_f32(shape, synth.SEED_CONFIG[1])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    got = ctx.fd_hessian_features(img, mask)
    ref = oracle.fd_hessian_features(img, mask)
    assert_features_close(got, ref, mask)
    got_nomask = ctx.fd_hessian_features(img, None)
    assert_features_close(got_nomask, oracle.fd_hessian_features(img, None))
    pl = ctx.fd_hessian_features(img, mask, layout=ife.PLANAR)
    np.testing.assert_array_equal(np.moveaxis(pl, 0, -1), got)
    i16 = synth.volume_i16(shape, 3)
    assert_features_close(ctx.fd_hessian_features(i16, mask),
                          oracle.fd_hessian_features(i16.astype(np.float32), mask), mask)


def test_fd_gradient_features(ctx, oracle, synth):
    shape = (19, 23, 66)
    img = synth.volume_f32(shape, 8)
    m = (synth.mask_ellipsoids(shape) > 0).astype(np.float32)
    np.testing.assert_array_equal(ctx.fd_gradient_features(img, m),
                                  oracle.fd_gradient_features(img, m))


def test_mask_image_f64(ctx, oracle):
    rng = np.random.default_rng(3)
    img = rng.standard_normal(100003)
    m = (rng.random(100003) > 0.5).astype(np.float64) * 2.0
    np.testing.assert_array_equal(ctx.mask_image_f64(img, m, -7.5), oracle.mask_image_f64(img, m, -7.5))


# ---------------------------------------------------------------------------------
# error behaviour
# ---------------------------------------------------------------------------------
def test_short_axis_is_rejected_like_itk(ctx, ife):
    img = np.zeros((3, 8, 8), np.float32)
    with pytest.raises(ife.IfeError) as e:
        ctx.emphysema_features(img, None, [1.0])
    assert e.value.code == ife.E_SIZE and "at least 4" in str(e.value)
    with pytest.raises(ife.IfeError) as e:
        ctx.normalized_gaussian_convolution(img, np.ones_like(img), 1.0)
    assert e.value.code == ife.E_SIZE
    # no recursive filter on this path: short axes are fine
    assert ctx.hessian3d(img).shape == (3, 8, 8, 6)


def test_bad_arguments(ctx, ife):
    img = np.zeros((8, 8, 8), np.float32)
    with pytest.raises(ife.IfeError) as e:
        ctx.emphysema_features(img, None, [0.0])
    assert e.value.code == ife.E_ARG
    with pytest.raises(ife.IfeError) as e:
        ctx.emphysema_features(img, None, [1.0], spacing=(0.0, 1, 1))
    assert e.value.code == ife.E_ARG
    with pytest.raises(ife.IfeError):
        ctx.set_option(999, 1)


def test_new_entry_points_refuse_bad_arguments(ctx, ife):
    """Round-3 additions to the C-ABI: argument checks happen on the host, before any launch."""
    import torch
    a = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    b = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    gbs = ctx.measure_stream(1, b.data_ptr(), a.data_ptr(), a.numel() * 4, 2)
    assert gbs > 10.0
    assert ctx.measure_stream(0, b.data_ptr(), None, a.numel() * 4, 2) > 10.0
    for args in ((1, b.data_ptr(), None, 4096, 1),          # a copy needs a source
                 (0, b.data_ptr() + 4, None, 4096, 1),      # 16-byte alignment
                 (0, b.data_ptr(), None, 4100, 1),          # whole 16-byte pieces
                 (2, b.data_ptr(), a.data_ptr(), 4096, 1),  # unknown mode
                 (0, b.data_ptr(), None, 4096, 0)):         # at least one pass
        with pytest.raises(ife.IfeError) as e:
            ctx.measure_stream(*args)
        assert e.value.code == ife.E_ARG
    shape = (8, 8, 64)
    vol = torch.zeros(shape, dtype=torch.float32, device="cuda")
    out = torch.zeros(shape, dtype=torch.float32, device="cuda")
    ck = torch.zeros(ctx.stage_z_ck_bytes(shape), dtype=torch.uint8, device="cuda")
    st = torch.zeros(ife.Z_STATE_BYTES * 64 * 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ife.IfeError) as e:   # a neighbour below, but no incoming state
        ctx.stage_z_fused(0, [vol.data_ptr()], [out.data_ptr()], shape, (1, 1, 1), 0, 512, [1.0], True, False,
                          None, st.data_ptr(), [ck.data_ptr()])
    assert e.value.code == ife.E_ARG
    with pytest.raises(ife.IfeError) as e:   # in place
        ctx.stage_z_fused(1, [vol.data_ptr()], [vol.data_ptr()], shape, (1, 1, 1), 0, 512, [1.0], False, False,
                          None, st.data_ptr(), [ck.data_ptr()])
    assert e.value.code == ife.E_ARG
    with pytest.raises(ife.IfeError) as e:   # the quotient form runs on the strided axes only
        ctx.stage_recursive_gaussian_quotient([vol.data_ptr()], [vol.data_ptr()], [out.data_ptr()], shape,
                                              (1, 1, 1), 0, [1.0])
    assert e.value.code == ife.E_ARG


# ---------------------------------------------------------------------------------
# self-pinned golden files (tests/golden/make_golden.py)
# ---------------------------------------------------------------------------------
def test_golden_pipeline_snapshot_on_device(ctx):
    z = np.load(os.path.join(HERE, "golden", "pipeline_24x20x28.npz"))
    got = ctx.emphysema_features(z["image"], z["mask"], list(z["sigmas"]), tuple(z["spacing"]))
    for s in range(len(z["sigmas"])):
        assert_features_close(got[s], z["features"][s], z["mask"])


def test_golden_fd_snapshot_on_device(ctx):
    z = np.load(os.path.join(HERE, "golden", "fd_hessian_20.npz"))
    np.testing.assert_array_equal(ctx.hessian3d(z["image"]), z["hessian"])
    np.testing.assert_array_equal(ctx.gradient_magnitude(z["image"]), z["gradmag"])
    assert_features_close(ctx.fd_hessian_features(z["image"], z["mask"]), z["features"], z["mask"])


def test_golden_eigen_fixture_on_device(ctx):
    z = np.load(os.path.join(HERE, "golden", "eigen_f32.npz"))
    assert eig_rel_err(ctx.eigenvalues(z["A"]), z["ev_cmath"]) <= REL_TOL


# ---------------------------------------------------------------------------------
# opt-in variants: must stay inside the north_star bar, are NOT expected to be bit exact
# ---------------------------------------------------------------------------------
def test_fused_recurrence_option_stays_inside_the_bar(ctx, ife, oracle, synth):
    """IFE_OPT_IIR_FMA fuses each multiply-add of the recursive Gaussian.  The smoothed
    value may then differ from the reference arithmetic by one float ulp at rare voxels."""
    shape = (48, 52, 56)
    img = synth.volume_f32(shape, 31)
    mask = np.ones(shape, np.uint8)
    ctx.set_option(ife.OPT_IIR_FMA, 1)
    try:
        got = ctx.emphysema_features(img, mask, [1.0, 4.0])
    finally:
        ctx.set_option(ife.OPT_IIR_FMA, 0)
    for s, sigma in enumerate((1.0, 4.0)):
        ref = oracle.emphysema_features(img, mask, sigma)
        same = float((got[s][..., 0] == ref[..., 0]).mean())
        ulp = np.spacing(np.abs(ref[..., 0]))
        assert same > 0.9999 and (np.abs(got[s][..., 0] - ref[..., 0]) <= ulp).all()
        lam = np.maximum(np.abs(ref[..., 2]).astype(np.float64), 1e-30)
        err = np.abs(got[s][..., 2:5].astype(np.float64) - ref[..., 2:5]) / lam[..., None]
        assert np.quantile(err, 0.9999) <= 1e-5


@pytest.mark.parametrize("stride", [1, 2])
def test_checkpoint_stride_is_invisible(ctx, ife, oracle, synth, stride):
    shape = (70, 41, 45)
    img = synth.volume_f32(shape, 98)
    cert = np.ones(shape, np.float32)
    ctx.set_option(ife.OPT_IIR_CKPT, stride)
    try:
        got = ctx.normalized_gaussian_convolution(img, cert, 2.0)
    finally:
        ctx.set_option(ife.OPT_IIR_CKPT, 2)
    np.testing.assert_array_equal(got, oracle.normalized_gaussian_convolution(img, cert, 2.0))


def test_misaligned_device_pointers_are_refused(ctx, ife):
    """Vector stores on a misaligned pointer would fault on the device; the library answers
    IFE_E_ARG instead."""
    import torch
    shape = (8, 8, 8)
    img = torch.zeros(shape, dtype=torch.float32, device="cuda")
    buf = torch.zeros(8 * 8 * 8 * 8 + 4, dtype=torch.float32, device="cuda")
    with pytest.raises(ife.IfeError) as ei:
        ctx.emphysema_features_device(img.data_ptr(), ife.F32, None, ife.U8, shape, (1.0, 1.0, 1.0),
                                      [1.0], buf.data_ptr() + 4, ife.INTERLEAVED)
    assert ei.value.code == ife.E_ARG and "aligned" in str(ei.value)
    ctx.emphysema_features_device(img.data_ptr(), ife.F32, None, ife.U8, shape, (1.0, 1.0, 1.0),
                                  [1.0], buf.data_ptr() + 4, ife.PLANAR)   # 4-byte alignment suffices
    torch.cuda.synchronize()
