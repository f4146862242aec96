"""ife_scale_select on the device against tests/scale_select_oracle.py applied to the features that
ctx.emphysema_features (or ctx.differential_features) returns on the same device for the same
arguments; those features are held to the CPU oracle elsewhere.

IFE_SS_LAPLACIAN is one float product: response and index are compared bit for bit.  The three
Frangi kinds lie in [0, 1] and are three float expf factors, each a few 2^-24 off the float64
value: tol = 1e-5 absolute, the project's eigenvalue bar, leaves about a factor of ten.  With R[s]
the oracle's responses every voxel must satisfy: index 255 implies max R <= tol; otherwise
|response - R[index]| <= tol and R[index] >= max R - 2 tol.

The volume of 9 x 11 x 37 = 3663 voxels is no multiple of four, so three of its four feature planes
start off a 16-byte boundary and are read element by element, as are the rows of the outputs behind
the first; 8 x 11 x 37 = 3256 voxels is a multiple, and everything moves 16 bytes per lane.  Four
scales cross the group of three scales that the scale loop smooths together.

The fold launch does not cap its grid: a lane takes one group of four voxels and there is no
grid-stride loop, so there is no second trip to reach."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scale_select_oracle as Q  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (9, 11, 37)
SHAPE4 = (8, 11, 37)
SIGMAS = [1.0, 1.5, 2.0, 3.0]
TOL = 1e-5
GUARD = 64
FILL = 0xA5
KINDS = (Q.TUBE, Q.PLATE, Q.BLOB)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case(ctx, synth):
    """Image, mask, the device's features of the four scales (shared, never written) and c."""
    img = synth.volume_f32(SHAPE, 7)
    mask = (synth.mask_ellipsoids(SHAPE) > 0).astype(np.uint8)
    feats = ctx.emphysema_features(img, mask, SIGMAS)
    feats.setflags(write=False)
    return img, mask, feats, _median_c(feats, mask, SIGMAS)


def _median_c(feats, mask, sigmas):
    """The median over scales and foreground voxels of sigma^2 * Frobenius norm."""
    fg = mask.astype(bool) if mask is not None else np.ones(feats.shape[1:4], bool)
    return float(np.median(np.concatenate([np.float64(s) ** 2 * feats[k][..., 7][fg] for k, s in enumerate(sigmas)])))


def _ms(ife, dicts):
    return [ife.ScaleMeasure(**d) for d in dicts]


def _frangi(c, polarities=(1, -1), kinds=KINDS):
    return [Q.measure(k, p, 1.0, 0.5, 0.5, c) for k in kinds for p in polarities]


def _check_measure(resp, idx, feats, sigmas, m, mask=None, what=""):
    """One row of a result against the oracle; returns (R, max R) of the Frangi kinds."""
    assert resp.dtype == np.float32 and idx.dtype == np.uint8 and resp.shape == idx.shape == feats.shape[1:4]
    if mask is not None:
        assert (resp[mask == 0] == 0).all() and (idx[mask == 0] == Q.NONE).all(), what
    R = Q.responses(feats, sigmas, m)
    if m["kind"] == Q.LAPLACIAN:
        want, widx = Q.fold(R)
        assert want.dtype == np.float32
        assert np.array_equal(resp.view(np.uint32), want.view(np.uint32)), what
        assert np.array_equal(idx, widx), what
        return R, want
    assert not np.isnan(R).any()
    top = R.max(0)
    none = idx == Q.NONE
    assert (top[none] <= TOL).all() and (resp[none] == 0).all(), what          # no voxel is left out:
    chosen = np.take_along_axis(R, np.where(none, 0, idx)[None].astype(np.int64), 0)[0]
    err = np.abs(resp.astype(np.float64) - chosen)[~none]                       # every one is none or chosen
    print("%s kind %d polarity %+d: %d voxels chose a scale, worst |response - R[index]| %.3g, worst gap to the "
          "best scale %.3g" % (what, m["kind"], m["polarity"], int((~none).sum()), err.max() if err.size else 0.0,
                               (top - chosen)[~none].max() if err.size else 0.0))
    assert (idx[~none] < len(sigmas)).all(), what
    assert (err <= TOL).all(), what
    assert (chosen[~none] >= top[~none] - 2 * TOL).all(), what
    return R, top


def _check_all(ife, got, feats, sigmas, dicts, mask=None, what=""):
    resp, idx = got
    assert resp.shape[0] == idx.shape[0] == len(dicts)
    return [_check_measure(resp[k], idx[k], feats, sigmas, m, mask, what) for k, m in enumerate(dicts)]


# ---- the measures ------------------------------------------------------------------------------------
def test_laplacian_is_exact(ife, ctx, case):
    img, mask, feats, _ = case
    dicts = [Q.measure(Q.LAPLACIAN, p, g) for g in (1.0, 0.75) for p in (1, -1)]
    got = ctx.scale_select(img, mask, SIGMAS, _ms(ife, dicts))
    _check_all(ife, got, feats, SIGMAS, dicts, mask, "laplacian")
    resp, idx = got
    for k in range(4):   # both polarities answer somewhere, and every scale wins somewhere
        assert set(np.unique(idx[k])) == {0, 1, 2, 3, Q.NONE}, k


@pytest.mark.parametrize("polarity", [1, -1])
def test_tube_plate_blob(ife, ctx, case, polarity):
    img, mask, feats, c = case
    dicts = _frangi(c, (polarity,))
    got = ctx.scale_select(img, mask, SIGMAS, _ms(ife, dicts))
    checked = _check_all(ife, got, feats, SIGMAS, dicts, mask, "frangi")
    resp, idx = got
    assert (resp >= 0).all() and (resp <= 1).all()
    # so that the index check is not vacuous: few voxels have their two best scales within 2 tol,
    for k, (R, top) in enumerate(checked):
        live = top > 2 * TOL
        two = np.sort(R, 0)[-2:]
        share = float(((two[1] - two[0] <= 2 * TOL) & live).sum()) / max(int(live.sum()), 1)
        print("kind %d polarity %+d: %d live voxels, near-tie share %.4f, argmax histogram %s"
              % (dicts[k]["kind"], polarity, int(live.sum()), share,
                 np.bincount(idx[k][idx[k] != Q.NONE], minlength=4).tolist()))
        assert live.sum() > 30 and share <= 0.02, (dicts[k], share)     # the dark blob has the fewest, 45 on the CPU
    # and TUBE (bright) and PLATE choose each of the four scales somewhere
    if polarity == 1:
        for k in (0, 1):
            assert set(np.unique(idx[k])) >= {0, 1, 2, 3}, dicts[k]


# ---- measure count and order ---------------------------------------------------------------------------
def test_measure_count_and_order(ife, ctx, case):
    img, mask, feats, c = case
    dicts = [Q.measure(Q.PLATE, 1, 1.0, 0.5, 0.5, c), Q.measure(Q.LAPLACIAN, -1, 0.75), Q.measure(Q.BLOB, -1, 1.0, 0.5, 0.5, c),
             Q.measure(Q.TUBE, 1, 0.75, 0.4, 0.6, c)]
    resp, idx = ctx.scale_select(img, mask, SIGMAS, _ms(ife, dicts))
    for k, d in enumerate(dicts):           # four calls of one measure
        r1, i1 = ctx.scale_select(img, mask, SIGMAS, _ms(ife, [d]))
        assert r1.shape == (1,) + SHAPE
        assert np.array_equal(r1[0].view(np.uint32), resp[k].view(np.uint32)) and np.array_equal(i1[0], idx[k]), k
    r2, i2 = ctx.scale_select(img, mask, SIGMAS, _ms(ife, dicts[:2]))
    assert np.array_equal(r2.view(np.uint32), resp[:2].view(np.uint32)) and np.array_equal(i2, idx[:2])
    r3, i3 = ctx.scale_select(img, mask, SIGMAS, _ms(ife, dicts), want_index=False)    # scale_index = NULL
    assert i3 is None and np.array_equal(r3.view(np.uint32), resp.view(np.uint32))
    r4, _ = ctx.scale_select(img, mask, SIGMAS, _ms(ife, dicts[2:3]), want_index=False)
    assert np.array_equal(r4[0].view(np.uint32), resp[2].view(np.uint32))


# ---- scale counts --------------------------------------------------------------------------------------
def test_one_scale(ife, ctx, case):
    img, mask, feats, c = case
    dicts = [Q.measure(Q.LAPLACIAN, 1, 1.0)] + _frangi(c, (1,))
    got = ctx.scale_select(img, mask, SIGMAS[2:3], _ms(ife, dicts))
    _check_all(ife, got, feats[2:3], SIGMAS[2:3], dicts, mask, "one scale")
    assert set(np.unique(got[1])) == {0, Q.NONE}


def test_seven_scales_span_three_groups(ife, ctx, case):
    img, mask, _, c = case
    sigmas = [1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 3.5]
    feats = ctx.emphysema_features(img, mask, sigmas)
    dicts = [Q.measure(Q.LAPLACIAN, 1, 1.0), Q.measure(Q.LAPLACIAN, -1, 0.75)] + _frangi(c, (1,), (Q.TUBE, Q.PLATE))
    got = ctx.scale_select(img, mask, sigmas, _ms(ife, dicts))
    _check_all(ife, got, feats, sigmas, dicts, mask, "seven scales")
    assert {0, 3, 6} <= set(np.unique(got[1][0]))           # the first scale of every group wins somewhere


def test_a_repeated_sigma_never_wins(ife, ctx, case):
    img, mask, _, c = case
    sigmas = [1.0, 2.0, 1.0, 2.0, 3.0, 2.0]                  # the repeats sit in the same and in the next group
    dicts = [Q.measure(Q.LAPLACIAN, 1, 1.0)] + _frangi(c, (1,))
    resp, idx = ctx.scale_select(img, mask, sigmas, _ms(ife, dicts))
    assert not np.isin(idx, (2, 3, 5)).any()
    assert {0, 1, 4, Q.NONE} == set(np.unique(idx[0]))
    feats = ctx.emphysema_features(img, mask, sigmas)
    _check_all(ife, (resp, idx), feats, sigmas, dicts, mask, "repeated")


# ---- DEVICE memory -------------------------------------------------------------------------------------
def _device_bytes(torch_dev, payload, offset=0, fill=FILL):
    """A device byte buffer [guard | offset | payload | guard], all other bytes `fill`; returns
    (tensor, pointer of the payload, slice of the payload)."""
    torch, dev = torch_dev
    raw = np.full(GUARD + offset + len(payload) + GUARD, fill, np.uint8)
    raw[GUARD + offset:GUARD + offset + len(payload)] = np.frombuffer(payload, np.uint8)
    t = torch.from_numpy(raw).to(dev)
    torch.cuda.synchronize()
    return t, t.data_ptr() + GUARD + offset, slice(GUARD + offset, GUARD + offset + len(payload))


def _read(t, sl, dtype):
    return t.cpu().numpy()[sl].view(dtype)


def _guards_intact(t, sl, fill=FILL):
    h = t.cpu().numpy()
    return (h[:sl.start] == fill).all() and (h[sl.stop:] == fill).all()


def _device_call(ife, ctx, torch_dev, img, mask, sigmas, ms, roff, ioff, want_index=True):
    n = img.size
    ti, iptr, _ = _device_bytes(torch_dev, img.tobytes())
    tm, mptr, _ = _device_bytes(torch_dev, mask.tobytes()) if mask is not None else (None, None, None)
    assert iptr % 16 == 0
    tr, rptr, rsl = _device_bytes(torch_dev, bytes([0x5A]) * (4 * n * len(ms)), offset=4 * roff)
    tx, xptr, xsl = _device_bytes(torch_dev, bytes([0x5A]) * (n * len(ms)), offset=ioff)
    mdt = ife.U8 if mask is None or mask.dtype == np.uint8 else ife.U16
    idt = ife.F32 if img.dtype == np.float32 else ife.I16
    ctx.scale_select_device(iptr, idt, mptr, mdt, img.shape, (1.0, 1.0, 1.0), sigmas, ms, rptr,
                            xptr if want_index else None)
    assert _guards_intact(tr, rsl) and _guards_intact(tx, xsl)
    resp = _read(tr, rsl, np.float32).reshape((len(ms),) + img.shape)
    idx = _read(tx, xsl, np.uint8).reshape((len(ms),) + img.shape)
    if not want_index:
        assert (idx == 0x5A).all()
    return resp, idx


@pytest.mark.parametrize("roff", [0, 1, 2, 3])
def test_device_outputs_at_every_alignment(ife, ctx, torch_dev, case, roff):
    """The response at float offsets 0 .. 3 and the index at byte offsets 0 .. 3 from a 16-byte
    boundary, between guards; the results are the HOST call's."""
    img, mask, _, c = case
    dicts = [Q.measure(Q.LAPLACIAN, 1, 0.75), Q.measure(Q.TUBE, 1, 1.0, 0.5, 0.5, c), Q.measure(Q.PLATE, -1, 1.0, 0.5, 0.5, c)]
    ms = _ms(ife, dicts)
    want = ctx.scale_select(img, mask, SIGMAS, ms)
    for ioff in range(4):
        resp, idx = _device_call(ife, ctx, torch_dev, img, mask, SIGMAS, ms, roff, ioff)
        assert np.array_equal(resp.view(np.uint32), want[0].view(np.uint32)), (roff, ioff)
        assert np.array_equal(idx, want[1]), (roff, ioff)
    resp, _ = _device_call(ife, ctx, torch_dev, img, mask, SIGMAS, ms, roff, 0, want_index=False)
    assert np.array_equal(resp.view(np.uint32), want[0].view(np.uint32))


def test_device_outputs_of_a_volume_of_whole_pieces(ife, ctx, torch_dev, synth):
    """3256 voxels: every plane and every output row starts where the first does, so the aligned
    call moves 16 bytes per lane throughout and the others fall back row by row."""
    img = synth.volume_f32(SHAPE4, 7)
    mask = (synth.mask_ellipsoids(SHAPE4) > 0).astype(np.uint8)
    feats = ctx.emphysema_features(img, mask, SIGMAS)
    c = _median_c(feats, mask, SIGMAS)
    dicts = [Q.measure(Q.LAPLACIAN, -1, 1.0)] + _frangi(c, (1,))
    ms = _ms(ife, dicts)
    want = ctx.scale_select(img, mask, SIGMAS, ms)
    _check_all(ife, want, feats, SIGMAS, dicts, mask, "whole pieces")
    for roff, ioff in ((0, 0), (1, 0), (0, 1), (2, 3), (3, 2)):
        resp, idx = _device_call(ife, ctx, torch_dev, img, mask, SIGMAS, ms, roff, ioff)
        assert np.array_equal(resp.view(np.uint32), want[0].view(np.uint32)), (roff, ioff)
        assert np.array_equal(idx, want[1]), (roff, ioff)


# ---- input and mask variants, shapes, the differential path ----------------------------------------------
def test_int16_image_uint16_mask_and_no_mask(ife, ctx, synth, case):
    _, mask, _, _ = case
    i16 = synth.volume_i16(SHAPE, 7)
    for image, msk in ((i16, mask), (case[0], mask.astype(np.uint16)), (case[0], None), (i16, None)):
        feats = ctx.emphysema_features(image, msk, SIGMAS)
        c = _median_c(feats, msk, SIGMAS)
        dicts = [Q.measure(Q.LAPLACIAN, 1, 1.0)] + _frangi(c, (1,), (Q.TUBE, Q.PLATE)) + [Q.measure(Q.BLOB, -1, 1.0, 0.5, 0.5, c)]
        got = ctx.scale_select(image, msk, SIGMAS, _ms(ife, dicts))
        _check_all(ife, got, feats, SIGMAS, dicts, msk, "%s image, %s mask" % (image.dtype, msk.dtype if msk is not None else "no"))
        assert (got[1] != Q.NONE).sum() > 100


@pytest.mark.parametrize("shape", [(5, 5, 37), (4, 4, 5), (4, 4, 4), SHAPE4])
def test_small_shapes(ife, ctx, synth, shape):
    """925 voxels (odd), rows of five voxels, and 64 voxels: the smallest volume the feature calls
    take, a quarter of one wave of the fold."""
    img = synth.volume_f32(shape, 7)
    feats = ctx.emphysema_features(img, None, SIGMAS)
    c = _median_c(feats, None, SIGMAS)
    dicts = [Q.measure(Q.LAPLACIAN, 1, 1.0), Q.measure(Q.LAPLACIAN, -1, 1.0)] + _frangi(c, (1,), (Q.TUBE, Q.PLATE))
    got = ctx.scale_select(img, None, SIGMAS, _ms(ife, dicts))
    _check_all(ife, got, feats, SIGMAS, dicts, None, str(shape))
    assert ((got[1][0] != Q.NONE) | (got[1][1] != Q.NONE)).sum() > got[1][0].size // 2


@pytest.mark.parametrize("shape", [(3, 5, 37), (2, 3, 2)])
def test_shapes_below_four_voxels_are_the_feature_calls_refusal(ife, ctx, synth, shape):
    """The features are those of ife_emphysema_features, whose recursive Gaussian needs four voxels
    along every axis: it refuses these two shapes with IFE_E_SIZE, and so does the selection, with
    nothing written."""
    img = synth.volume_f32(shape, 7)
    with pytest.raises(ife.IfeError) as e:
        ctx.emphysema_features(img, None, SIGMAS)
    assert e.value.code == ife.E_SIZE
    lib = ife.load_library()
    d = ife._desc(shape, (1.0, 1.0, 1.0))
    ms = (ife.ScaleMeasure * 1)(ife.ScaleMeasure(ife.SS_LAPLACIAN))
    resp, idx = np.full(img.size, 9, np.float32), np.full(img.size, 9, np.uint8)
    rc = lib.ife_scale_select(ctx._h, img.ctypes.data, ife.F32, None, ife.U8, C.byref(d), ife._sigma_arg(SIGMAS), 4, ms, 1,
                              resp.ctypes.data, idx.ctypes.data, ife.MEM_HOST)
    assert rc == ife.E_SIZE and (resp == 9).all() and (idx == 9).all()


def test_differential_path(ife, ctx, case):
    img, mask, _, _ = case
    ctx.set_option(ife.OPT_DIFFERENTIAL, 1)
    try:
        feats = ctx.differential_features(img, mask, SIGMAS)
        c = _median_c(feats, mask, SIGMAS)
        dicts = [Q.measure(Q.LAPLACIAN, 1, 1.0), Q.measure(Q.LAPLACIAN, -1, 0.75)] + _frangi(c, (1,), (Q.TUBE, Q.PLATE))
        got = ctx.scale_select(img, mask, SIGMAS, _ms(ife, dicts))
        more = ctx.scale_select(img, mask, SIGMAS, _ms(ife, _frangi(c, (-1,)) + [Q.measure(Q.BLOB, 1, 1.0, 0.5, 0.5, c)]))
    finally:
        ctx.set_option(ife.OPT_DIFFERENTIAL, 0)
    _check_all(ife, got, feats, SIGMAS, dicts, mask, "differential")
    _check_all(ife, more, feats, SIGMAS, _frangi(c, (-1,)) + [Q.measure(Q.BLOB, 1, 1.0, 0.5, 0.5, c)], mask, "differential")
    assert (got[1][0] != Q.NONE).sum() > 100
    # and it is another path: not the finite-difference features
    fd = ctx.scale_select(img, mask, SIGMAS, _ms(ife, dicts[:1]))
    assert not np.array_equal(fd[0][0], got[0][0])


# ---- refusals -------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_context_alone(ife, ctx, torch_dev, case):
    img, mask, _, c = case
    n = img.size
    lib = ife.load_library()
    d = ife._desc(SHAPE, (1.0, 1.0, 1.0))
    ti, iptr, _ = _device_bytes(torch_dev, img.tobytes())
    tm, mptr, _ = _device_bytes(torch_dev, mask.tobytes())
    tr, rptr, rsl = _device_bytes(torch_dev, bytes([0x5A]) * (16 * n))
    tx, xptr, xsl = _device_bytes(torch_dev, bytes([0x5A]) * (4 * n))
    good = dict(kind=ife.SS_TUBE, polarity=1, gamma=1.0, alpha=0.5, beta=0.5, c=c)
    nan, inf = float("nan"), float("inf")

    def call(measures, n_measures=None, sigmas=SIGMAS, response=rptr, mem=ife.MEM_DEVICE, null_measures=False):
        arr = (ife.ScaleMeasure * max(len(measures), 1))(*[ife.ScaleMeasure(**m) for m in measures])
        rc = lib.ife_scale_select(ctx._h, iptr, ife.F32, mptr, ife.U8, C.byref(d), ife._sigma_arg(sigmas), len(sigmas),
                                  None if null_measures else arr, len(measures) if n_measures is None else n_measures,
                                  response, xptr, mem)
        return rc, lib.ife_last_error(ctx._h).decode()

    refused = [
        (dict(measures=[good], n_measures=0), "n_measures"), (dict(measures=[good] * 5), "n_measures"),
        (dict(measures=[good], n_measures=-1), "n_measures"),
        (dict(measures=[good], sigmas=[1.0] * 256), "n_sigmas"),
        (dict(measures=[good, dict(good, kind=4)]), "measures[1]: kind"), (dict(measures=[dict(good, kind=-1)]), "measures[0]: kind"),
        (dict(measures=[dict(good, polarity=0)]), "polarity"), (dict(measures=[dict(good, polarity=2)]), "polarity"),
        (dict(measures=[dict(good, gamma=-0.5)]), "gamma"), (dict(measures=[dict(good, gamma=nan)]), "gamma"),
        (dict(measures=[dict(good, gamma=inf)]), "gamma"),
        (dict(measures=[dict(good, kind=ife.SS_LAPLACIAN, gamma=-1.0)]), "gamma"),
        (dict(measures=[dict(good, alpha=0.0)]), "alpha"), (dict(measures=[dict(good, alpha=nan)]), "alpha"),
        (dict(measures=[dict(good, kind=ife.SS_PLATE, beta=-1.0)]), "beta"), (dict(measures=[dict(good, beta=inf)]), "beta"),
        (dict(measures=[good, good, dict(good, kind=ife.SS_BLOB, c=0.0)]), "measures[2]: c"),
        (dict(measures=[dict(good, c=inf)]), "c must"),
        (dict(measures=[good], null_measures=True), "measures"),
        (dict(measures=[good], response=None), "null"), (dict(measures=[good], response=rptr + 2), "response"),
        (dict(measures=[good], mem=7), "mem"), (dict(measures=[good], sigmas=[1.0, 0.0]), "sigma"),
    ]
    for kwargs, word in refused:
        rc, text = call(**kwargs)
        assert rc == ife.E_ARG and word in text, (kwargs, rc, text)
    assert (_read(tr, rsl, np.uint8) == 0x5A).all() and (_read(tx, xsl, np.uint8) == 0x5A).all()
    assert _guards_intact(tr, rsl) and _guards_intact(tx, xsl)
    # LAPLACIAN ignores alpha, beta and c; and the context is as usable as before
    rc, text = call([dict(good, kind=ife.SS_LAPLACIAN, alpha=nan, beta=-1.0, c=0.0), good])
    assert rc == ife.OK, text
    want = ctx.scale_select(img, mask, SIGMAS, [ife.ScaleMeasure(ife.SS_LAPLACIAN), ife.ScaleMeasure(**good)])
    got = _read(tr, rsl, np.float32)[:2 * n].reshape((2,) + SHAPE)
    assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(_read(tx, xsl, np.uint8)[:2 * n].reshape((2,) + SHAPE), want[1])
    assert (_read(tr, rsl, np.uint8)[8 * n:] == 0x5A).all() and (_read(tx, xsl, np.uint8)[2 * n:] == 0x5A).all()
