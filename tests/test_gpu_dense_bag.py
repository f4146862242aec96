"""The dense bag on the device (ife_dense_rois, ife_dense_roi_histograms, ife_bag_image_dense):
one region per mask voxel whose box fits the volume (include/ife/ROI/DenseROIGenerator.hxx:24-46),
counted by sliding box sums instead of box by box.

The checker throughout is oracle.roi_histograms applied to a box list built in numpy by the
generator's rule; the per-box device path (ctx.roi_histograms / ctx.bag_image on the same list) is
the second witness.  Everything is integer counting: counts must be EQUAL, not close.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def dense_boxes(gen, size):
    """DenseROIGenerator::generate: np.nonzero walks z, y, x, which is raster order."""
    sx, sy, sz = size
    nz, ny, nx = gen.shape
    boxes = []
    for z, y, x in zip(*np.nonzero(gen)):
        x0, y0, z0 = x - sx // 2, y - sy // 2, z - sz // 2
        if x0 >= 0 and y0 >= 0 and z0 >= 0 and x0 + sx <= nx and y0 + sy <= ny and z0 + sz <= nz:
            boxes.append((x0, y0, z0, sx, sy, sz))
    return np.array(boxes, np.int64).reshape(-1, 6)


def labels(shape, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 3, shape).astype(np.uint8)
    m[: shape[0] // 4] = 0
    return m


def size3(size):
    return (C.c_int64 * 3)(*[int(v) for v in size])


# ---- ife_dense_rois --------------------------------------------------------------------------
def block_mask(dtype, with_centre=True):
    lab = np.zeros((10, 12, 14), dtype)
    lab[3:7, 2:9, 4:11] = 2 if dtype == np.uint8 else 700
    lab[0, 0, 0] = 1                    # a mask voxel whose box fits only for size (1, 1, 1)
    if not with_centre:
        lab[5, 6, 7] = 0                # the one centre of the whole-volume box
    return lab


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("size", [(5, 3, 3), (4, 2, 6), (1, 1, 1), (14, 12, 10), (15, 3, 3)])
def test_dense_rois_match_the_generator_rule(ctx, dtype, size):
    lab = block_mask(dtype)
    want = dense_boxes(lab, size)
    got = ctx.dense_rois(lab, size)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    if size == (5, 3, 3):
        assert len(want) == 4 * 7 * 7
    if size == (1, 1, 1):
        assert len(want) == 4 * 7 * 7 + 1
    if size == (14, 12, 10):            # the whole volume: one region or none
        assert len(want) == 1
        assert ctx.dense_rois(block_mask(dtype, with_centre=False), size).shape == (0, 6)
    if size == (15, 3, 3):              # larger than the volume: zero regions and no error
        assert len(want) == 0


def test_dense_rois_count_only_and_capacity(ctx, ife):
    lib = ife.load_library()
    lab = block_mask(np.uint16)
    want = dense_boxes(lab, (4, 2, 6))
    d = ife._desc(lab.shape, (1.0, 1.0, 1.0))
    n = C.c_int64(-1)
    rc = lib.ife_dense_rois(ctx._h, lab.ctypes.data, ife.U16, C.byref(d), size3((4, 2, 6)), C.byref(n), None, 0,
                            ife.MEM_HOST)
    assert rc == ife.OK and n.value == len(want) > 1
    buf = np.full((len(want) - 1, 6), -7, np.int64)
    n = C.c_int64(-1)
    rc = lib.ife_dense_rois(ctx._h, lab.ctypes.data, ife.U16, C.byref(d), size3((4, 2, 6)), C.byref(n),
                            buf.ctypes.data, buf.shape[0], ife.MEM_HOST)
    assert rc == ife.E_SIZE and n.value == len(want)      # the count is still reported
    assert np.all(buf == -7)                              # and nothing was written
    assert np.array_equal(ctx.dense_rois(lab, (4, 2, 6)), want)


# ---- ife_dense_roi_histograms ------------------------------------------------------------------
def special_features(rng, shape, ncomp):
    """One decimal, so that values land on edges; a few NaN, +-inf and -0.0."""
    feat = np.round(rng.normal(0, 3, shape + (ncomp,)), 1).astype(np.float32)
    flat = feat.reshape(-1)
    pos = rng.choice(flat.size, 64, replace=False)
    flat[pos[:16]] = np.nan
    flat[pos[16:32]] = np.inf
    flat[pos[32:48]] = -np.inf
    flat[pos[48:]] = -0.0
    return feat


def test_dense_roi_histograms_both_layouts(ctx, ife, oracle):
    rng = np.random.default_rng(61)
    shape, size = (12, 18, 70), (41, 5, 4)     # wider than one wave, the last row segment partial
    feat = special_features(rng, shape, 8)
    m = labels(shape, 62)
    edges = np.sort(np.round(rng.normal(0, 3, (8, 13)), 1).astype(np.float32), axis=1)
    boxes = dense_boxes(m, size)
    assert len(boxes) > 1000
    want, _ = oracle.roi_histograms(feat, np.minimum(m, 1), boxes, edges)
    got = ctx.dense_roi_histograms(feat, m, size, edges)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(got, ctx.roi_histograms(feat, m, boxes, edges))
    planar = np.ascontiguousarray(np.moveaxis(feat, -1, 0))
    got_p = ctx.dense_roi_histograms(planar, m.astype(np.uint16), size, edges, layout=ife.PLANAR)
    assert np.array_equal(got_p, want)


def test_dense_roi_histograms_generating_mask(ctx, ife, oracle):
    rng = np.random.default_rng(63)
    shape, size = (18, 22, 26), (7, 5, 6)
    feat = special_features(rng, shape, 8)
    m = labels(shape, 64)
    m[:9] = 0                                   # boxes around z = 3 hold no mask voxel
    gen = (rng.integers(0, 4, shape) == 0).astype(np.uint16) * 9
    gen[3, 10, 12] = 9
    edges = np.sort(np.round(rng.normal(0, 3, (8, 13)), 1).astype(np.float32), axis=1)
    boxes = dense_boxes(gen, size)
    centres = boxes[:, :3] + np.array(size) // 2
    assert np.any(m[centres[:, 2], centres[:, 1], centres[:, 0]] == 0)     # centres outside the counting mask
    want, _ = oracle.roi_histograms(feat, np.minimum(m, 1), boxes, edges)
    empty = np.flatnonzero(want.reshape(len(boxes), -1).sum(1) == 0)
    assert empty.size >= 1
    got = ctx.dense_roi_histograms(feat, m, size, edges, gen_mask=gen)
    assert np.array_equal(got, want)
    assert not got[empty].any()
    assert np.array_equal(got, ctx.roi_histograms(feat, m, boxes, edges))
    # the counting mask as its own generating mask is the default
    assert np.array_equal(ctx.dense_roi_histograms(feat, m, size, edges),
                          ctx.dense_roi_histograms(feat, m, size, edges, gen_mask=m))


@pytest.mark.parametrize("n_edges,scratch_mb", [(1, 0), (254, 0), (254, 1)])
def test_dense_roi_histograms_edge_counts(ctx, ife, oracle, n_edges, scratch_mb):
    """One edge, and the most one byte per voxel allows; with the scratch bounded to 1 MiB the
    255 bins go through the passes in groups (18*22*26 voxels * (1 + 3*255) bytes do not fit)."""
    rng = np.random.default_rng(65)
    shape, size = (18, 22, 26), (7, 5, 6)
    feat = special_features(rng, shape, 2)
    m = labels(shape, 66)
    edges = np.sort(np.round(rng.normal(0, 3, (2, n_edges)), 2).astype(np.float32), axis=1)
    boxes = dense_boxes(m, size)
    want, _ = oracle.roi_histograms(feat, np.minimum(m, 1), boxes, edges)
    ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, scratch_mb)
    try:
        got = ctx.dense_roi_histograms(feat, m, size, edges)
    finally:
        ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, 0)
    assert got.shape == (len(boxes), 2, n_edges + 1)
    assert np.array_equal(got, want)


# ---- ife_bag_image_dense -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def bag_case(oracle, synth):
    shape, sigmas, size = (24, 28, 32), [1.0, 2.0], (9, 9, 7)
    img = synth.volume_f32(shape, 77)
    lab = synth.mask_ellipsoids(shape)
    clamped = np.minimum(lab, 1).astype(np.uint8)
    feats = [oracle.emphysema_features(img, clamped, s) for s in sigmas]
    # histogram specification: equalizing edges of the whole foreground, 9 bins
    edges = np.stack([oracle.equalized_edges(oracle.sort_f32(f[..., c][clamped != 0]), 9)
                      for f in feats for c in range(8)])
    boxes = dense_boxes(lab, size)
    want = [oracle.roi_histograms(f, clamped, boxes, edges[i * 8:(i + 1) * 8])[0] for i, f in enumerate(feats)]
    return dict(img=img, lab=lab, sigmas=sigmas, size=size, edges=edges, boxes=boxes, want=want)


@pytest.mark.parametrize("scratch_mb", [0, 1])
def test_bag_image_dense_matches_per_box_path_and_oracle(ctx, ife, bag_case, scratch_mb):
    """scratch_mb = 1: one scale at a time and the 9 bins in two groups; same counts."""
    b = bag_case
    assert set(np.unique(b["lab"])) == {0, 1, 2} and len(b["boxes"]) > 100
    ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, scratch_mb)
    try:
        got = ctx.bag_image_dense(b["img"], b["lab"], b["sigmas"], b["size"], b["edges"])
    finally:
        ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, 0)
    assert got.shape == (len(b["boxes"]), 16, 9)
    for i, want in enumerate(b["want"]):
        assert np.array_equal(got[:, i * 8:(i + 1) * 8, :], want), i
    if scratch_mb == 0:
        assert np.array_equal(got, ctx.bag_image(b["img"], b["lab"], b["sigmas"], b["boxes"], b["edges"]))


def test_bag_image_dense_generating_mask(ctx, bag_case):
    b = bag_case
    gen = (b["lab"] == 2).astype(np.uint16)
    boxes = dense_boxes(gen, b["size"])
    assert 0 < len(boxes) < len(b["boxes"])
    got = ctx.bag_image_dense(b["img"], b["lab"], b["sigmas"], b["size"], b["edges"], gen_mask=gen)
    assert np.array_equal(got, ctx.bag_image(b["img"], b["lab"], b["sigmas"], boxes, b["edges"]))


# ---- errors, and the context after them ----------------------------------------------------------
def test_dense_errors_leave_the_context_usable(ctx, ife, synth):
    lib = ife.load_library()
    rng = np.random.default_rng(67)
    shape, size = (10, 12, 14), (5, 3, 3)
    feat = rng.normal(0, 3, shape + (2,)).astype(np.float32)
    img = synth.volume_f32(shape, 68)
    m = block_mask(np.uint8)
    edges = np.sort(rng.normal(0, 3, (2, 300)).astype(np.float32), axis=1)
    bag_edges = np.sort(rng.normal(0, 300, (8, 300)).astype(np.float32), axis=1)
    d = ife._desc(shape, (1.0, 1.0, 1.0))
    sig = (C.c_float * 1)(1.0)
    counts = np.full(64, 0xdeadbeef, np.uint32)     # capacity 0: no call below may write a row
    want_hist = ctx.roi_histograms(feat, m, dense_boxes(m, size), edges[:, :5])
    want_bag = ctx.bag_image(img, m, [1.0], dense_boxes(m, size), bag_edges[:, :5])

    def hist(size=size, n_edges=5, mask=m.ctypes.data):
        n = C.c_int64(-1)
        return lib.ife_dense_roi_histograms(ctx._h, feat.ctypes.data, ife.INTERLEAVED, 2, mask, ife.U8, None, ife.U8,
                                            C.byref(d), size3(size), edges.ctypes.data, n_edges, counts.ctypes.data,
                                            0, C.byref(n), ife.MEM_HOST)

    def bag(size=size, n_edges=5, mask=m.ctypes.data):
        n = C.c_int64(-1)
        return lib.ife_bag_image_dense(ctx._h, img.ctypes.data, ife.F32, mask, ife.U8, None, ife.U8, C.byref(d), sig,
                                       1, size3(size), bag_edges.ctypes.data, n_edges, counts.ctypes.data, 0,
                                       C.byref(n), ife.MEM_HOST)

    def rois(size=size, mask=m.ctypes.data):
        n = C.c_int64(-1)
        return lib.ife_dense_rois(ctx._h, mask, ife.U8, C.byref(d), size3(size), C.byref(n), None, 0, ife.MEM_HOST)

    def still_usable():
        assert np.array_equal(ctx.dense_roi_histograms(feat, m, size, edges[:, :5]), want_hist)
        assert np.array_equal(ctx.bag_image_dense(img, m, [1.0], size, bag_edges[:, :5]), want_bag)

    still_usable()
    cases = [
        ("size 0", dict(size=(5, 0, 3)), ife.E_ARG),
        ("negative size", dict(size=(-1, 3, 3)), ife.E_ARG),
        ("no edges", dict(n_edges=0), ife.E_ARG),
        ("more edges than one byte holds", dict(n_edges=255), ife.E_ARG),
        ("null mask", dict(mask=None), ife.E_ARG),
        ("sx beyond one byte", dict(size=(256, 1, 1)), ife.E_SIZE),
        ("sx*sy beyond two bytes", dict(size=(255, 258, 1)), ife.E_SIZE),
        ("sx*sy*sz beyond four bytes", dict(size=(255, 257, 65538)), ife.E_SIZE),
    ]
    for what, kw, code in cases:
        for call in (hist, bag):
            assert call(**kw) == code, (what, call.__name__)
            assert ife.load_library().ife_last_error(ctx._h)
            still_usable()
        if "n_edges" not in kw and code == ife.E_ARG:
            assert rois(**kw) == code, what
            still_usable()
    assert np.all(counts == 0xdeadbeef)
    # inside the bounds, larger than the volume: zero regions, no error
    assert hist(size=(255, 257, 65537)) == ife.OK and hist(size=(101, 101, 101)) == ife.OK
    assert ctx.dense_roi_histograms(feat, m, (41, 41, 41), edges[:, :5]).shape == (0, 2, 6)
    # more regions than rows: E_SIZE, nothing written
    assert hist() == ife.E_SIZE and bag() == ife.E_SIZE and np.all(counts == 0xdeadbeef)
    still_usable()
