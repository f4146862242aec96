"""IFE_OPT_DIFFERENTIAL: the composite calls (sample columns, bag rows, dense bag, dense stream, scale
stream) on the differential feature path.  The contract is a composition of calls that exist
without the option and are checked against the oracle elsewhere: with the option at 1 every call
gives bit for bit what its documented composition gives when ife_differential_features stands in
for ife_emphysema_features.  So there is no tolerance here, except in the one test that compares
the sample kernel with the CPU oracle directly; everything else is compared as uint32 or on integers.

Neither new kernel caps its grid (jet_samples_kernel: one wave per row segment, jet_codes_kernel_*:
one lane per piece or voxel), so there is no second trip to cross."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.parity import assert_eig_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jet_oracle  # noqa: E402
import niftiio  # noqa: E402
import test_gpu_dense_stream as dense_stream  # noqa: E402  (its base case and its frequencies)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "image-feature-extraction_amd", "host")
BIN = os.path.join(HOST, "bin")

SHAPES = [(5, 7, 9), (6, 5, 70), (4, 4, 130)]
SPACING = (0.7, 1.3, 2.0)
SIGMAS = [1.0, 1.7]
FOREGROUNDS = [(1,), (2, 3), (1, 2, 3)]
TOL_MODE0 = 1e-6   # the eigenvalue bar of trig mode 0, as in tests/test_gpu_differential.py

# the row segments of 64 voxels: a partial one only; a full one and one of 6 lanes; two full ones
# and one of 2 lanes -- and n % 4 = 3, 0, 0
assert [nx % 64 for _, _, nx in SHAPES] == [9, 6, 2] and [nx // 64 for _, _, nx in SHAPES] == [0, 1, 2]
assert [nz * ny * nx % 4 for nz, ny, nx in SHAPES] == [3, 0, 0]


@pytest.fixture(scope="module", autouse=True)
def option_back_to_zero(ctx, ife):
    """The session-wide context never leaves this file with the option set."""
    yield
    ctx.set_option(ife.OPT_DIFFERENTIAL, 0)
    ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, 0)


@contextlib.contextmanager
def differential(ctx, ife, scratch_mb=0):
    ctx.set_option(ife.OPT_DIFFERENTIAL, 1)
    ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, scratch_mb)
    try:
        yield ctx
    finally:
        ctx.set_option(ife.OPT_DIFFERENTIAL, 0)
        ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_labels(shape, seed=7):
    """uint16 labels {0, 1, 2, 3}: noise, then whole rows of one value -- a row of 0 (its segments hold
    no sample for any foreground set: the wave that returns early), a row of 1 and a row of 2 (fully
    sampled segments for the sets with 1 and for (2, 3)) and a row of 3 between rows of noise."""
    nz, ny, nx = shape
    lab = np.random.default_rng(seed).integers(0, 4, shape).astype(np.uint16)
    lab[0, 0, :] = 0
    lab[1, 1, :] = 1
    lab[1, 2, :] = 2
    lab[2, 3, :] = 3
    assert set(np.unique(lab)) == {0, 1, 2, 3}
    assert not (lab[2, 3] == lab[2, 2]).all() and not (lab[2, 3] == lab[3, 3]).all()
    return lab


def clamp(lab):
    return np.minimum(lab, 1).astype(np.uint8)


_cases = {}


def case(ctx, synth, shape, kind="f32", mode=0):
    """Two images over one label volume and F = ctx.differential_features of each with the clamped
    labels (what the composite calls hand over), computed once per (shape, kind, trig mode)."""
    key = (shape, kind, mode)
    if key not in _cases:
        make = synth.volume_f32 if kind == "f32" else synth.volume_i16
        lab = make_labels(shape)
        imgs = [make(shape, 610), make(shape, 611)]
        feats = [ctx.differential_features(im, clamp(lab), SIGMAS, SPACING) for im in imgs]
        for a in imgs + feats + [lab]:
            a.setflags(write=False)
        _cases[key] = (imgs, lab, feats)
    return _cases[key]


def expected_columns(feats, lab, fg):
    """Column (scale i, component c): F_i[..., c] at the voxels whose label is in fg, raster order,
    image after image."""
    sel = np.isin(lab, fg)
    return [np.concatenate([f[i][..., c][sel] for f in feats]) for i in range(len(SIGMAS)) for c in range(8)]


def assert_columns(samples, want, what):
    assert samples.count() == len(want[0]) > 0
    for c, w in enumerate(want):
        got = samples.column(c)
        assert np.array_equal(bits(got), bits(w)), "%s: column %d" % (what, c)


# ---- 1. samples, all-foreground branch -----------------------------------------------------------
@pytest.mark.parametrize("fg", FOREGROUNDS, ids=lambda f: "fg" + "".join(map(str, f)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_samples_all_foreground(ctx, ife, synth, shape, fg):
    imgs, lab, feats = case(ctx, synth, shape)
    sel = np.isin(lab, fg)
    segs = sel.reshape(-1, shape[2])[:, :64]
    assert (~segs.any(axis=1)).any() and segs.all(axis=1).any()      # a skipped wave, a full segment
    with differential(ctx, ife):
        s = ctx.samples(8 * len(SIGMAS))
        try:
            s.add_image(imgs[0], lab, SIGMAS, foreground=fg, spacing=SPACING)
            first = s.count()
            assert first == int(sel.sum()) > 0
            s.add_image(imgs[1], lab, SIGMAS, foreground=fg, spacing=SPACING)    # behind a non-zero offset
            assert s.count() == 2 * first
            assert_columns(s, expected_columns(feats, lab, fg), "%s fg %s" % (shape, fg))
        finally:
            s.close()


def test_samples_all_foreground_int16_image(ctx, ife, synth):
    shape, fg = SHAPES[1], (2, 3)
    imgs, lab, feats = case(ctx, synth, shape, "i16")
    assert imgs[0].dtype == np.int16
    with differential(ctx, ife):
        s = ctx.samples(8 * len(SIGMAS))
        try:
            for im in imgs:
                s.add_image(im, lab, SIGMAS, foreground=fg, spacing=SPACING)
            assert_columns(s, expected_columns(feats, lab, fg), "int16")
        finally:
            s.close()


def test_samples_all_foreground_default_trig_mode(ctx_fast, ife, synth):
    shape, fg = SHAPES[2], (1, 2, 3)
    imgs, lab, feats = case(ctx_fast, synth, shape, mode=2)
    mode0 = case(ctx_fast, synth, shape)[2] if (shape, "f32", 0) in _cases else None
    with differential(ctx_fast, ife):
        s = ctx_fast.samples(8 * len(SIGMAS))
        try:
            for im in imgs:
                s.add_image(im, lab, SIGMAS, foreground=fg, spacing=SPACING)
            assert_columns(s, expected_columns(feats, lab, fg), "trig mode 2")
        finally:
            s.close()
    if mode0 is not None:   # the two modes do differ somewhere, so this test sees the context's mode
        assert not np.array_equal(bits(mode0[0]), bits(feats[0]))


def test_samples_all_foreground_device_memory(ctx, ife, synth):
    import torch
    shape, fg = SHAPES[1], (1,)
    imgs, lab, feats = case(ctx, synth, shape)
    d_lab = torch.from_numpy(lab.view(np.int16).copy()).cuda()      # the same 16 bits
    with differential(ctx, ife):
        s = ctx.samples(8 * len(SIGMAS))
        try:
            for im in imgs:
                d_img = torch.from_numpy(np.array(im)).cuda()
                s.add_image_device(d_img.data_ptr(), ife.F32, d_lab.data_ptr(), ife.U16, shape, SIGMAS,
                                   foreground=fg, spacing=SPACING)
                ctx.synchronize()
            assert_columns(s, expected_columns(feats, lab, fg), "device")
        finally:
            s.close()


# ---- 2. samples against the CPU oracle -------------------------------------------------------------
def test_samples_against_the_oracle(ctx, ife, synth, oracle):
    """The chain above rests on the product's own ife_differential_features; this one does not: the
    gathered rows against the same gather of jet_oracle.features.  S and G as bits, the eigenvalue
    components at the 1e-6 bar of tests/test_gpu_differential.py."""
    shape, fg, sigma = (6, 5, 70), (1, 2, 3), 1.5
    img = synth.volume_f32(shape, 612)
    lab = make_labels(shape)
    ref = jet_oracle.features(oracle, img, clamp(lab), sigma, SPACING)
    want = ref[np.isin(lab, fg)]
    with differential(ctx, ife):
        s = ctx.samples(8)
        try:
            s.add_image(img, lab, [sigma], foreground=fg, spacing=SPACING)
            got = np.stack([s.column(c) for c in range(8)], axis=1)
        finally:
            s.close()
    assert got.shape == want.shape and got.shape[0] > 64
    assert np.array_equal(bits(got[:, 0]), bits(want[:, 0])), "S"
    assert np.array_equal(bits(got[:, 1]), bits(want[:, 1])), "G"
    assert_eig_parity(got, want, TOL_MODE0, "samples 6 x 5 x 70")


# ---- 3. samples, sampled branch ----------------------------------------------------------------------
def test_samples_sampled_branch(ctx, ife, synth):
    shape = SHAPES[1]
    imgs, lab, feats = case(ctx, synth, shape)
    n = lab.size
    rng = np.random.default_rng(3)
    idx = np.stack([np.concatenate([[0, n - 1, n - 1, 0, 17, 17], rng.integers(0, n, 50)]) for _ in SIGMAS])
    assert idx.shape == (len(SIGMAS), 56) and not np.array_equal(idx[0], idx[1])
    with differential(ctx, ife):
        s = ctx.samples(8 * len(SIGMAS))
        try:
            s.add_image(imgs[0], lab, SIGMAS, foreground=(1,), indices=idx, spacing=SPACING)
            for i in range(len(SIGMAS)):
                for c in range(8):
                    want = feats[0][i][..., c].reshape(-1)[idx[i]]
                    assert np.array_equal(bits(s.column(i * 8 + c)), bits(want)), (i, c)
        finally:
            s.close()


# ---- 4. bag_image ---------------------------------------------------------------------------------------
def edges_of(ctx, feats, clamped, nbins):
    """Equalizing edges of the given features over the mask: populated bins on this path."""
    return np.stack([ctx.equalized_edges(ctx.sort_f32(f[..., c][clamped != 0]), nbins)
                     for f in feats for c in range(8)])


def test_bag_image(ctx, ife, synth):
    shape = SHAPES[1]
    nz, ny, nx = shape
    imgs, lab, feats = case(ctx, synth, shape)
    clamped = clamp(lab)
    edges = edges_of(ctx, feats[0], clamped, 6)
    rois = np.array([[0, 0, 0, 9, 3, 4], [nx - 7, ny - 2, nz - 3, 7, 2, 3], [30, 1, 2, 40, 4, 4], [0, 0, 0, nx, ny, nz]],
                    np.int64)                                       # all of them touch the border
    with differential(ctx, ife):
        got = ctx.bag_image(imgs[0], lab, SIGMAS, rois, edges, spacing=SPACING)
    assert got.shape == (4, 16, 6) and got.sum() > 0
    for i in range(len(SIGMAS)):
        want = ctx.roi_histograms(feats[0][i], clamped, rois, edges[8 * i:8 * i + 8], spacing=SPACING)
        assert np.array_equal(got[:, 8 * i:8 * i + 8], want), "scale %d" % i
    fd = ctx.bag_image(imgs[0], lab, SIGMAS, rois, edges, spacing=SPACING)
    assert not np.array_equal(fd, got)                              # the option is what made the difference


# ---- 5. / 6. the dense bag and its stream -------------------------------------------------------------
DENSE_SIGMAS, DENSE_NBINS = dense_stream.SIGMAS, dense_stream.NBINS


def dense_case(ctx, synth, shape, size, base):
    c = dense_stream.make_case(ctx, synth, shape, size, 501, base=base)
    clamped = clamp(c["lab"])
    feats = ctx.differential_features(c["img"], clamped, DENSE_SIGMAS)
    c["edges"] = edges_of(ctx, feats, clamped, DENSE_NBINS)
    c["want"] = np.concatenate([ctx.dense_roi_histograms(feats[i], clamped, size, c["edges"][8 * i:8 * i + 8],
                                                         gen_mask=c["gen"]) for i in range(len(DENSE_SIGMAS))], axis=1)
    return c


@pytest.fixture(scope="module")
def dense_base(ctx, synth):
    """The base case of tests/test_gpu_dense_stream.py (14 x 12 x 70, box 5 x 3 x 4, a generating mask,
    two scales, 5 bins) with edges from the differential features; `want` is the composition."""
    c = dense_case(ctx, synth, (14, 12, 70), (5, 3, 4), True)
    assert c["img"].size % 4 == 0 and c["want"].shape == (6000, 16, DENSE_NBINS)
    return c


@pytest.fixture(scope="module")
def dense_odd(ctx, synth):
    """n % 4 = 3: the plane stride of the codes is odd, jet_codes_kernel_scalar takes every voxel."""
    c = dense_case(ctx, synth, (9, 7, 11), (3, 3, 2), False)
    assert c["img"].size % 4 == 1 or c["img"].size % 4 == 3
    return c


@pytest.mark.parametrize("scratch_mb", [0, 1])
def test_bag_image_dense(ctx, ife, dense_base, scratch_mb):
    c = dense_base
    with differential(ctx, ife, scratch_mb):
        got = ctx.bag_image_dense(c["img"], c["lab"], DENSE_SIGMAS, c["size"], c["edges"], gen_mask=c["gen"])
    assert got.dtype == np.uint32 and np.array_equal(got, c["want"])
    assert (c["want"].sum(-1) > 0).any()


def test_bag_image_dense_scalar_codes(ctx, ife, dense_odd):
    c = dense_odd
    with differential(ctx, ife):
        got = ctx.bag_image_dense(c["img"], c["lab"], DENSE_SIGMAS, c["size"], c["edges"], gen_mask=c["gen"])
        blocks = list(ctx.bag_image_dense_stream(c["img"], c["lab"], DENSE_SIGMAS, c["size"], c["edges"],
                                                 gen_mask=c["gen"], values="counts"))
    assert len(c["want"]) > 0 and np.array_equal(got, c["want"])
    assert np.array_equal(dense_stream.joined(blocks, len(c["want"])), c["want"])


@pytest.mark.parametrize("scratch_mb", [0, 1])
def test_dense_stream(ctx, ife, dense_base, scratch_mb):
    """Under the bound of 1 MiB an eighth of what labels (11 760 bytes) and codes (188 160) leave is
    106 082 bytes = 331 rows of 320 bytes, less than the 600 of a plane: one plane per block."""
    c = dense_base
    out = {}
    with differential(ctx, ife, scratch_mb):
        for values in ("counts", "frequencies"):
            out[values] = list(ctx.bag_image_dense_stream(c["img"], c["lab"], DENSE_SIGMAS, c["size"], c["edges"],
                                                          gen_mask=c["gen"], values=values))
    for blocks in out.values():
        assert len(blocks) == 1 if scratch_mb == 0 else len(blocks) >= 3
    counts = dense_stream.joined(out["counts"], len(c["want"]))
    assert counts.dtype == np.uint32 and np.array_equal(counts, c["want"])
    dense_stream.assert_frequencies(dense_stream.joined(out["frequencies"], len(c["want"])), c["want"])


# ---- 7. the scale stream ---------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["INTERLEAVED", "PLANAR"])
def test_scale_stream(ctx, ife, synth, layout):
    """The value of the option at _begin decides for the whole stream (include/ife_hip.h)."""
    shape = SHAPES[1]
    imgs, lab, _ = case(ctx, synth, shape)
    lay = getattr(ife, layout)
    want = {1: ctx.differential_features(imgs[0], lab, SIGMAS, SPACING, layout=lay),    # the caller's mask,
            0: ctx.emphysema_features(imgs[0], lab, SIGMAS, SPACING, layout=lay)}       # not a clamped one
    assert not np.array_equal(bits(want[0]), bits(want[1]))
    try:
        for value in (1, 0):
            ctx.set_option(ife.OPT_DIFFERENTIAL, value)
            got = list(ctx.emphysema_features_stream(imgs[0], lab, SIGMAS, SPACING, layout=lay))
            assert len(got) == len(SIGMAS)
            for i, g in enumerate(got):
                assert np.array_equal(bits(g), bits(want[value][i])), (value, i)
        for value in (1, 0):                                 # the other value before the second _fetch
            ctx.set_option(ife.OPT_DIFFERENTIAL, value)
            it = ctx.emphysema_features_stream(imgs[0], lab, SIGMAS, SPACING, layout=lay)
            first = next(it)                                 # _begin and _fetch(0)
            ctx.set_option(ife.OPT_DIFFERENTIAL, 1 - value)
            rest = list(it)                                  # _fetch(1), _end
            for i, g in enumerate([first] + rest):
                assert np.array_equal(bits(g), bits(want[value][i])), ("opened under", value, i)
    finally:
        ctx.set_option(ife.OPT_DIFFERENTIAL, 0)


# ---- 8. the rules of the option -----------------------------------------------------------------------------
def test_option_rules(ctx, ife, synth):
    for bad in (2, -1):
        with pytest.raises(ife.IfeError) as e:
            ctx.set_option(ife.OPT_DIFFERENTIAL, bad)
        assert e.value.code == ife.E_ARG
    with ife.Multi([0, 0]) as m:
        with pytest.raises(ife.IfeError) as e:
            m.set_option(ife.OPT_DIFFERENTIAL, 1)
        assert e.value.code == ife.E_ARG and "one device" in str(e.value)
        m.set_option(ife.OPT_DIFFERENTIAL, 0)
    shape = SHAPES[0]
    imgs, lab, _ = case(ctx, synth, shape)
    clamped = clamp(lab)
    fd = ctx.emphysema_features(imgs[0], clamped, SIGMAS, SPACING)
    edges = edges_of(ctx, fd, clamped, 4)
    rois = np.array([[0, 0, 0, 9, 7, 5], [2, 1, 1, 5, 4, 3]], np.int64)
    ctx.set_option(ife.OPT_DIFFERENTIAL, 1)
    ctx.set_option(ife.OPT_DIFFERENTIAL, 0)
    got = ctx.bag_image(imgs[0], lab, SIGMAS, rois, edges, spacing=SPACING)
    for i in range(len(SIGMAS)):
        want = ctx.roi_histograms(fd[i], clamped, rois, edges[8 * i:8 * i + 8], spacing=SPACING)
        assert np.array_equal(got[:, 8 * i:8 * i + 8], want)


# ---- 9. four scales through every sink, on both paths ----------------------------------------------------------
FOUR_SIGMAS = [1.0, 1.3, 1.7, 2.2]


@pytest.mark.parametrize("option", [0, 1], ids=["finite_differences", "differential"])
def test_four_scales_through_every_sink(ctx, ife, synth, dense_base, option):
    """More scales than one group of the finite-difference loop holds (three): the fourth scale comes
    from a second group, which finds the sources where the first left them and writes behind the
    columns, volumes and codes of three scales.  Every composite call against the volume call of the
    same path, which tests/test_gpu_z_sweep.py holds to the oracle at four and five scales; all as
    uint32 or on integers."""
    shape, fg = SHAPES[1], (1, 2, 3)
    img, lab = synth.volume_f32(shape, 630), make_labels(shape)
    clamped, sel = clamp(lab), np.isin(lab, fg)
    volume_call = ctx.differential_features if option else ctx.emphysema_features
    want = volume_call(img, clamped, FOUR_SIGMAS, SPACING)
    assert len(want) == 4 and int(sel.sum()) > 64
    c = dense_base
    dense_clamped = clamp(c["lab"])
    edges = edges_of(ctx, volume_call(c["img"], dense_clamped, FOUR_SIGMAS), dense_clamped, DENSE_NBINS)
    assert edges.shape == (32, DENSE_NBINS - 1)
    dense_args = (c["img"], c["lab"])
    ctx.set_option(ife.OPT_DIFFERENTIAL, option)
    try:
        s = ctx.samples(32)
        try:
            s.add_image(img, lab, FOUR_SIGMAS, foreground=fg, spacing=SPACING)
            assert_columns(s, [want[i][..., k][sel] for i in range(4) for k in range(8)], "four scales")
        finally:
            s.close()
        fetched = list(ctx.emphysema_features_stream(img, clamped, FOUR_SIGMAS, SPACING))
        single = [ctx.bag_image_dense(*dense_args, [FOUR_SIGMAS[i]], c["size"], edges[8 * i:8 * i + 8], gen_mask=c["gen"])
                  for i in range(4)]
        bag = ctx.bag_image_dense(*dense_args, FOUR_SIGMAS, c["size"], edges, gen_mask=c["gen"])
        blocks = list(ctx.bag_image_dense_stream(*dense_args, FOUR_SIGMAS, c["size"], edges, gen_mask=c["gen"],
                                                 values="counts"))
    finally:
        ctx.set_option(ife.OPT_DIFFERENTIAL, 0)
    assert len(fetched) == 4
    for i in range(4):
        assert np.array_equal(bits(fetched[i]), bits(want[i])), "scale stream, scale %d" % i
    assert bag.dtype == np.uint32 and bag.shape == (len(c["want"]), 32, DENSE_NBINS)
    streamed = dense_stream.joined(blocks, len(bag))
    assert streamed.dtype == np.uint32
    for i in range(4):
        assert single[i].shape == (len(bag), 8, DENSE_NBINS) and (single[i].sum(-1) > 0).any()
        assert np.array_equal(bag[:, 8 * i:8 * i + 8], single[i]), "dense bag, scale %d" % i
        assert np.array_equal(streamed[:, 8 * i:8 * i + 8], single[i]), "dense stream, scale %d" % i


# ---- 10. the tools under IFE_DIFFERENTIAL ---------------------------------------------------------------------
TOOL_SHAPE, TOOL_SCALES, TOOL_NBINS = (12, 20, 24), [1.0, 2.5], 5


def run_tool(tool, args, differential_env, devices=None):
    env = dict(os.environ)
    for k in ("IFE_DIFFERENTIAL", "IFE_DEVICES", "IFE_DENSE_STREAM", "IFE_DENSE_BLOCK_MB"):
        env.pop(k, None)
    if differential_env:
        env["IFE_DIFFERENTIAL"] = "1"
    if devices:
        env["IFE_DEVICES"] = devices
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, env=env)


@pytest.fixture(scope="module")
def tools(ctx, synth, tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "image-feature-extraction_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    d = tmp_path_factory.mktemp("differential_tools")
    img = synth.volume_f32(TOOL_SHAPE, 620)
    lab = synth.mask_ellipsoids(TOOL_SHAPE).astype(np.uint16)
    clamped = clamp(lab)
    niftiio.write(str(d / "img.nii.gz"), img)
    niftiio.write(str(d / "lab.nii.gz"), lab)
    niftiio.write(str(d / "mask.nii.gz"), clamped)
    feats = ctx.differential_features(img, clamped, TOOL_SCALES)
    edges = edges_of(ctx, feats, clamped, TOOL_NBINS)
    (d / "hist.txt").write_text("".join(",".join("%.9g" % v for v in row) + "\n" for row in edges))
    edges = np.array([[np.float32(float("%.9g" % v)) for v in row] for row in edges], np.float32)
    rois = np.array([[0, 0, 0, 9, 8, 7], [24 - 9, 20 - 8, 12 - 7, 9, 8, 7], [5, 6, 2, 12, 9, 6]], np.int64)
    (d / "rois.txt").write_text("index size\n" + "".join("[%d, %d, %d][%d, %d, %d]\n" % tuple(r) for r in rois))
    (d / "pairs.csv").write_text("%s , %s\n" % (d / "img.nii.gz", d / "lab.nii.gz"))
    os.mkdir(str(d / "out"))
    return dict(dir=d, img=img, lab=lab, clamped=clamped, feats=feats, edges=edges, rois=rois)


def row_text(freq_row):
    return ["%g" % v for v in freq_row.ravel()]


def tool_row(line):
    return [t.replace("-nan", "nan") for t in line.split(",")]


def scale_args():
    return [a for s in TOOL_SCALES for a in ("-s", "%g" % s)]


def test_edges_tool(ctx, ife, tools):
    t, d = tools, tools["dir"]
    tool = "DetermineHistogramBinEdges_MultiScaleEigenvalueFeatures"
    text = {}
    for on in (True, False):
        out = d / ("edges%d.txt" % on)
        r = run_tool(tool, ["-i", d / "pairs.csv", "-o", out, "-b", TOOL_NBINS, "-S", 0, "-f", 1, "-f", 2] + scale_args(), on)
        assert r.returncode == 0, r.stderr
        text[on] = out.read_text().splitlines()[2:]
    with differential(ctx, ife):
        s = ctx.samples(16)
        try:
            s.add_image(t["img"], t["lab"].astype(np.uint8), TOOL_SCALES, foreground=(1, 2))
            want = s.equalized_edges(TOOL_NBINS)
        finally:
            s.close()
    assert text[True] == [",".join("%g" % v for v in row) for row in want]
    assert text[False] != text[True]


def test_makebag_tools(ctx, ife, tools):
    t, d = tools, tools["dir"]
    size = (5, 3, 3)
    with differential(ctx, ife):
        bag = ctx.bag_image(t["img"], t["lab"], TOOL_SCALES, t["rois"], t["edges"])
        dense = ctx.bag_image_dense(t["img"], t["lab"], TOOL_SCALES, size, t["edges"])
    assert len(dense) > 100
    text = {}
    for on in (True, False):
        r = run_tool("MakeBag", ["-i", d / "img.nii.gz", "-m", d / "lab.nii.gz", "-H", d / "hist.txt", "-o", d / "out",
                                 "-r", d / "rois.txt", "-p", "bag%d" % on] + scale_args(), on)
        assert r.returncode == 0, r.stderr
        r = run_tool("MakeBagDense", ["-i", d / "img.nii.gz", "-m", d / "lab.nii.gz", "-H", d / "hist.txt", "-o",
                                      d / "out", "-x", size[0], "-y", size[1], "-z", size[2], "-p", "dense%d" % on]
                     + scale_args(), on)
        assert r.returncode == 0, r.stderr
        text[on] = ((d / "out" / ("bag%d.bag" % on)).read_text().splitlines(),
                    (d / "out" / ("dense%d.bag" % on)).read_text().splitlines())
    rows, dense_rows = text[True]
    assert len(rows) == len(t["rois"]) and len(dense_rows) == len(dense)
    assert tool_row(rows[1]) == row_text(dense_stream.frequencies(bag[1])[0])
    j = len(dense) // 2
    assert tool_row(dense_rows[j]) == row_text(dense_stream.frequencies(dense[j])[0])
    assert text[False][0] != rows and text[False][1] != dense_rows


def test_extract_features_tool_streams_the_differential_path(ife, tools):
    t, d = tools, tools["dir"]
    r = run_tool("ExtractFeatures", ["-i", d / "img.nii.gz", "-m", d / "mask.nii.gz", "-o", d / "feat"] + scale_args(), True)
    assert r.returncode == 0, r.stderr
    for i, sigma in enumerate(TOOL_SCALES):
        for c, name in enumerate(ife.FEATURE_NAMES):
            vol, _ = niftiio.read(str(d / "feat") + "_scale_%.6f%s.nii.gz" % (sigma, name))
            assert np.array_equal(bits(vol), bits(t["feats"][i][..., c])), (sigma, name)


def test_tools_refuse_several_devices(tools):
    d = tools["dir"]
    common = ["-i", d / "img.nii.gz", "-m", d / "lab.nii.gz", "-H", d / "hist.txt", "-o", d / "out"] + scale_args()
    runs = {"ExtractFeatures": ["-i", d / "img.nii.gz", "-m", d / "mask.nii.gz", "-o", d / "multi"] + scale_args(),
            "DetermineHistogramBinEdges_MultiScaleEigenvalueFeatures":
                ["-i", d / "pairs.csv", "-o", d / "multi.txt", "-b", TOOL_NBINS, "-S", 0, "-f", 1] + scale_args(),
            "MakeBag": common + ["-r", d / "rois.txt", "-p", "multi"],
            "MakeBagDense": common + ["-x", 5, "-y", 3, "-z", 3, "-p", "multidense"]}
    for tool, args in runs.items():
        r = run_tool(tool, args, True, devices="0,0")
        assert r.returncode == 1, (tool, r.stdout, r.stderr)
        assert "the differential convolution runs on one device" in r.stderr, (tool, r.stderr)
