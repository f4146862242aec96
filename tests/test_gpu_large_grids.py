"""The second trip of every capped grid and the chunk hand-over of every two-level scan.

A launch of min(work, cap) workgroups loops, and a scan over chunks of 4096 entries carries an
offset from one workgroup to the next; at the shapes of the other test files (a few thousand
voxels) neither happens.  Every test here names the cap or chunk size its shape crosses and where
the constant lives, and asserts the crossing with the literal number, so that a later change of
the shape cannot drop the coverage unnoticed.

The checkers are the ones the small tests use: oracle.pyoracle, tests/jet_oracle.py,
tests/edt_oracle.py and numpy.  A test on more than about a million voxels runs in a context of
its own, so that the session context's workspace and staging buffers stay small."""
import math
import os
import sys

import numpy as np
import pytest

from oracle.parity import assert_eig_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_oracle as E  # noqa: E402
import jet_oracle  # noqa: E402
from test_gpu_dense_bag import dense_boxes  # noqa: E402  (the generator's rule in numpy)

pytestmark = pytest.mark.gpu

TOL_MODE0 = 1e-6        # the eigenvalue bar of trig mode 0 (tests/test_gpu_differential.py)


def _to_device(array):
    """A device copy (the shared inputs are read-only arrays, which torch does not wrap)."""
    import torch
    return torch.from_numpy(np.array(array)).cuda()


def _own_context(ife):
    c = ife.Context(0)
    c.set_option(ife.OPT_TRIG_MODE, 0)
    return c


# ---- 1. the differential path beyond one grid ---------------------------------------------------
# csrc/diff_capi.inc launch_jet: jet_kernel_vec4 and jet_kernel_scalar run min(work, 256 * 8 = 2048)
# workgroups of 256 lanes; a lane of the vec4 kernel takes a piece of four voxels.
# csrc/ife_capi.hip launch_prep: prep_kernel_scalar runs at most 8192 workgroups of 256 lanes.
JET_SHAPE, JET_SPACING, JET_SIGMA = (132, 128, 132), (0.7, 1.3, 2.0), 1.5
JET_N = 132 * 128 * 132
assert JET_N == 2230272 and JET_N % 4 == 0
assert JET_N // 4 > 2048 * 256          # jet_kernel_vec4: a second trip over the pieces
assert JET_N > 4 * 2048 * 256           # jet_kernel_scalar on the whole volume: five trips
assert JET_N > 8192 * 256               # prep_kernel_scalar on the whole volume: a second trip


def _jet_mask(synth, kind):
    """"ellipsoids": synth.mask_ellipsoids clamped to 1, whose last foreground plane is z = 115 of
    132, so that the last 133 120 voxels (the second trip of the vec4 kernel, the fifth of the scalar
    one) lie outside it and only the zero stores are seen there.  "rolled": the same mask 40 planes
    further along z, which puts foreground and background into those voxels."""
    mask = np.minimum(synth.mask_ellipsoids(JET_SHAPE), 1).astype(np.uint8)
    last = mask.reshape(-1)[4 * 2048 * 256:]
    if kind == "rolled":
        mask = np.ascontiguousarray(np.roll(mask, 40, axis=0))
        last = mask.reshape(-1)[4 * 2048 * 256:]
        assert last.any() and not last.all()
    else:
        assert not last.any()
    assert 0 < np.count_nonzero(mask) < mask.size
    return mask


@pytest.fixture(scope="module", params=["ellipsoids", "rolled"])
def jet_case(request, ife, synth, oracle):
    """Image, mask, the oracle's features and the host-mode interleaved result: computed once per
    mask, shared, never written to."""
    img = synth.volume_f32(JET_SHAPE, synth.SEED_CONFIG[3])
    mask = _jet_mask(synth, request.param)
    ref = jet_oracle.features(oracle, img, mask, JET_SIGMA, JET_SPACING)
    with _own_context(ife) as c:
        host = c.differential_features(img, mask, [JET_SIGMA], JET_SPACING)[0]
    for a in (img, mask, ref, host):
        a.setflags(write=False)
    return img, mask, ref, host


def test_differential_features_vec4_second_trip(jet_case):
    """Host mode, interleaved: staged buffers are aligned and n % 4 == 0, so jet_kernel_vec4 takes
    all 557 568 pieces with 524 288 lanes."""
    img, mask, ref, host = jet_case
    assert img.size % 4 == 0 and img.size // 4 > 2048 * 256
    np.testing.assert_array_equal(host[..., 0], ref[..., 0], "S")
    np.testing.assert_array_equal(host[..., 1], ref[..., 1], "G")
    assert_eig_parity(host, ref, TOL_MODE0, "132 x 128 x 132")
    assert (host[mask == 0].view(np.uint32) == 0).all(), "not zero outside the mask"


def test_differential_features_device_planar_second_trip(ife, jet_case):
    """Device mode, every pointer aligned, planar: the 16-byte plane stores of the second trip."""
    import torch
    img, mask, _, host = jet_case
    assert img.size % 4 == 0 and img.size // 4 > 2048 * 256
    d_img, d_mask = _to_device(img), _to_device(mask)
    d_out = torch.full((8,) + JET_SHAPE, float("nan"), dtype=torch.float32, device="cuda")
    assert d_img.data_ptr() % 16 == 0 and d_mask.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    with _own_context(ife) as c:
        c.differential_features_device(d_img.data_ptr(), ife.F32, d_mask.data_ptr(), ife.U8, JET_SHAPE, JET_SPACING,
                                       [JET_SIGMA], d_out.data_ptr(), layout=ife.PLANAR)
        c.synchronize()
        got = d_out.cpu().numpy()
    np.testing.assert_array_equal(np.moveaxis(got, 0, -1).view(np.uint32), host.view(np.uint32))


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_differential_features_scalar_kernels_many_trips(ife, jet_case, layout):
    """The mask one byte into a larger allocation: no 4-element form of the mask exists, so
    prep_kernel_scalar (8192 x 256 lanes) and jet_kernel_scalar (2048 x 256 lanes) take the whole
    volume, in two and in five trips."""
    import torch
    img, mask, _, host = jet_case
    assert img.size > 4 * 2048 * 256 and img.size > 8192 * 256
    d_img = _to_device(img)
    d_buf = torch.zeros(JET_N + 1, dtype=torch.uint8, device="cuda")
    d_buf[1:].copy_(_to_device(mask).reshape(-1))
    mask_ptr = d_buf.data_ptr() + 1
    assert mask_ptr % 4 == 1
    planar = layout == "planar"
    d_out = torch.full(((8,) + JET_SHAPE) if planar else (JET_SHAPE + (8,)), float("nan"), dtype=torch.float32,
                       device="cuda")
    torch.cuda.synchronize()
    with _own_context(ife) as c:
        c.differential_features_device(d_img.data_ptr(), ife.F32, mask_ptr, ife.U8, JET_SHAPE, JET_SPACING,
                                       [JET_SIGMA], d_out.data_ptr(), layout=ife.PLANAR if planar else ife.INTERLEAVED)
        c.synchronize()
        got = d_out.cpu().numpy()
    if planar:
        got = np.moveaxis(got, 0, -1)
    np.testing.assert_array_equal(got.view(np.uint32), host.view(np.uint32))


def test_jet_vec4_second_trip(ife, synth, oracle):
    """ife_normalized_convolution_jet, fractional certainty with 30 % exact zeros (as _certainty of
    tests/test_gpu_differential.py): the ten-component stores of the second trip."""
    img = synth.volume_f32(JET_SHAPE, synth.SEED_CONFIG[3])
    assert img.size % 4 == 0 and img.size // 4 > 2048 * 256
    rng = np.random.default_rng(8)
    cert = (rng.random(JET_SHAPE) * (rng.random(JET_SHAPE) >= 0.3)).astype(np.float32)
    want = jet_oracle.jet(oracle, img, cert, JET_SIGMA, JET_SPACING)
    with _own_context(ife) as c:
        got = c.normalized_convolution_jet(img, cert, JET_SIGMA, JET_SPACING)
    np.testing.assert_array_equal(got, want)


# ---- 3. the distance map beyond 2048 line blocks ------------------------------------------------
# csrc/distance_kernels.hpp EDT_MAX_LINE_BLOCKS = 2048 workgroups of 64 lanes, one lane per line
# (csrc/distance_capi.inc edt_line_blocks): a lane's second line reuses its candidate stack.
EDT_Z_SHAPE, EDT_Y_SHAPE = (3, 363, 363), (363, 3, 363)
assert 363 * 363 == 131769 > 2048 * 64          # lines of the z pass of EDT_Z_SHAPE: nx * ny
assert 363 * 363 > 2048 * 64                    # lines of the y pass of EDT_Y_SHAPE: nx * nz
EDT_SPACINGS = [(1.0, 1.0, 1.0), (0.5, 2.0, 1.0)]   # nothing rounds: bit for bit (tests/test_gpu_distance.py)


@pytest.mark.parametrize("spacing", EDT_SPACINGS, ids=["unit", "pow2"])
@pytest.mark.parametrize("shape", [EDT_Z_SHAPE, EDT_Y_SHAPE], ids=["z_pass", "y_pass"])
def test_distance_map_second_trip_of_the_line_kernel(ctx, shape, spacing):
    nz, ny, nx = shape
    assert max(nx * ny, nx * nz) > 2048 * 64
    mask = (np.random.default_rng(41).random(shape) < 0.02).astype(np.uint8)
    d2 = E.sq_dist(E.contour(mask != 0), spacing, slabs=True)
    for positive in (True, False):
        for squared in (False, True):
            got = ctx.signed_distance_map(mask, spacing, inside_is_positive=positive, squared=squared)
            val = d2 if squared else np.sqrt(d2)
            want = np.where((mask != 0) == positive, val, -val)
            bad = np.flatnonzero(got.ravel() != want.ravel())
            assert bad.size == 0, "positive=%s squared=%s: %d voxels differ, first %d: %r != %r" % (
                positive, squared, bad.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def test_expected_distance_many_lines(ctx):
    """131 769 z lines: the second trip of the line kernel in its reducing form, and 514 or 515
    partial sums per thread of edt_reduce_kernel (EDT_REDUCE_THREADS = 256)."""
    shape = EDT_Z_SHAPE
    assert shape[1] * shape[2] > 2048 * 64 and shape[1] * shape[2] > 256 * 514
    rng = np.random.default_rng(42)
    mask = ((rng.random(shape) < 0.6) * 3).astype(np.uint8)
    prob = rng.random(shape)
    dist = E.signed_distance_map(mask, slabs=True)              # once, for the terms and the replica
    terms = E.expected_distance_terms(mask, prob, dist=dist)
    n = int(np.count_nonzero(mask))
    assert terms.size == n and (terms >= 0).all()
    want = math.fsum(terms) / n
    got, got_n = ctx.expected_distance(mask, prob)
    again, again_n = ctx.expected_distance(mask, prob)
    replica, replica_n = E.expected_distance_device_order(mask, prob, dist=dist)
    print("expected distance: gpu %.17g oracle %.17g replica %.17g rel %.3g (bound %.3g)" % (
        got, want, replica, abs(got - want) / want, 2 * n * 2.0 ** -53))
    assert got_n == n == again_n == replica_n                    # the count is exact
    assert abs(got - want) <= 2 * n * 2.0 ** -53 * want          # the bound tests/test_gpu_distance.py derives
    assert np.float64(got).tobytes() == np.float64(again).tobytes()
    # the documented order, every step an IEEE double operation (built without contraction)
    assert np.float64(got).tobytes() == np.float64(replica).tobytes()


# csrc/distance_capi.inc edt_run: edt_x_kernel runs min(ny * nz, 1 << 20) workgroups of one wave,
# a row each; with more rows a workgroup takes a second one and overwrites its ballots in LDS.
EDT_X_SHAPE = (1025, 1024, 1)
assert 1025 * 1024 == 1049600 > 1 << 20          # rows of the x pass: ny * nz, of one voxel each
EDT_X_SITES = [    # (z, y): isolated voxels, each a site; row = z * ny + y
    [(0, 0), (3, 1000), (511, 77), (512, 512), (700, 1023), (1023, 1023), (1024, 0), (1024, 600), (1024, 1023)],
    [(0, 0), (1, 1), (200, 900), (640, 3), (900, 450), (1023, 0), (1024, 1), (1024, 333), (1024, 1022),
     (1022, 700)],
]


@pytest.fixture(scope="module")
def edt_x_context(ife):
    with ife.Context(0) as c:
        yield c


def test_distance_map_second_trip_of_the_x_kernel(edt_x_context):
    """Two site sets back to back on one context: rows that a missing second trip leaves unwritten
    cannot pass on what the call before left in the buffers.  The very first call sees a fresh
    allocation, so it is the later ones (the unsquared map of the same sites, whose values differ
    from the squared ones, and the second site set) that hold the second trip."""
    nz, ny, nx = EDT_X_SHAPE
    assert ny * nz > 1 << 20
    for sites in EDT_X_SITES:
        assert 8 <= len(sites) <= 12 and (0, 0) in sites
        assert sum(z * ny + y >= 1 << 20 for z, y in sites) >= 2
        mask = np.zeros(EDT_X_SHAPE, np.uint8)
        for z, y in sites:
            mask[z, y, 0] = 1
        site = E.contour(mask != 0)
        assert np.array_equal(site, mask != 0)
        d2 = E.sq_dist_allpairs(site)
        got = edt_x_context.signed_distance_map(mask, squared=True)
        want = np.where(mask != 0, d2, -d2)
        bad = np.flatnonzero(got.ravel() != want.ravel())
        assert bad.size == 0, "%d voxels differ, first %d: %r != %r" % (
            bad.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])
        got = edt_x_context.signed_distance_map(mask, inside_is_positive=False)
        assert np.array_equal(got, np.where(mask != 0, -np.sqrt(d2), np.sqrt(d2)))


def test_expected_distance_second_trip_of_the_x_kernel(edt_x_context):
    """Small squares of foreground; two of them reach the plane z = 1024, the rows of the second
    trip, where the ends of their edge are sites and the three voxels between are not (the face
    of the volume makes no site), so terms of the sum come from distances written on that trip."""
    nz, ny, nx = EDT_X_SHAPE
    assert ny * nz > 1 << 20
    mask = np.zeros(EDT_X_SHAPE, np.uint8)
    for z, y, edge in [(0, 0, 5), (300, 500, 7), (800, 1017, 7), (1020, 40, 5), (1020, 700, 5)]:
        mask[z:z + edge, y:y + edge, 0] = 2
    site = E.contour(mask != 0)
    assert mask[0].any() and site[1024].sum() == 4 and np.count_nonzero(mask[1024]) == 10
    dist = np.sqrt(E.sq_dist_allpairs(site))
    prob = np.random.default_rng(43).random(EDT_X_SHAPE)
    n = int(np.count_nonzero(mask))
    replica, replica_n = E.expected_distance_device_order(mask, prob, dist=dist)
    assert replica > 0
    got, got_n = edt_x_context.expected_distance(mask, prob)
    assert got_n == n == replica_n
    assert np.float64(got).tobytes() == np.float64(replica).tobytes()


# ---- 4. sample columns over many chunks --------------------------------------------------------------
# csrc/stats_kernels.hpp GATHER_CHUNK = 4096 voxels per workgroup of count_foreground_kernel and
# gather_foreground_kernel; scan_chunks_kernel: 256 threads, ceil(nchunks / 256) chunks each.
GATHER_N = 258 * 4096 + 17
assert (GATHER_N + 4095) // 4096 == 259 > 256          # scan_chunks_kernel: per = 2


def _column_filler(rng, n):
    return rng.normal(0, 1, n).astype(np.float32)


@pytest.mark.parametrize("form", ["interleaved_u8", "planar_u16"])
def test_samples_add_features_many_chunks(ife, form):
    """259 chunks, so a non-zero offset for all but the first and two chunks per thread of the
    scan; two adds, the second onto a non-zero col_offset and into grown columns.  The columns on
    both sides of the target hold samples of their own and keep them."""
    n = GATHER_N
    assert (n + 4095) // 4096 > 256
    rng = np.random.default_rng(51)
    lab = np.array([0, 1, 2, 5])[rng.integers(0, 4, n)]
    feat = rng.normal(0, 3, (1, 1, n, 2)).astype(np.float32)
    sel = np.isin(lab, (1, 2))
    want = [feat[0, 0, :, c][sel] for c in range(2)]             # raster order
    if form == "interleaved_u8":
        layout, f, m = ife.INTERLEAVED, feat, lab.astype(np.uint8).reshape(1, 1, n)
    else:
        layout, f, m = ife.PLANAR, np.ascontiguousarray(np.moveaxis(feat, -1, 0)), lab.astype(np.uint16).reshape(1, 1, n)
    left, right = _column_filler(rng, 1000), _column_filler(rng, 777)
    with _own_context(ife) as c:
        s = c.samples(4)
        s.add_features(0, left.reshape(1, 1, -1, 1), indices=np.arange(left.size))
        s.add_features(3, right.reshape(1, 1, -1, 1), indices=np.arange(right.size))
        for k in (1, 2):
            s.add_features(1, f, mask=m, foreground=(1, 2), layout=layout)
            assert s.count(1) == s.count(2) == k * int(sel.sum())
            assert s.count(0) == left.size and s.count(3) == right.size
            for col in range(2):
                assert np.array_equal(s.column(1 + col).view(np.uint32), np.tile(want[col], k).view(np.uint32)), (k, col)
            assert np.array_equal(s.column(0).view(np.uint32), left.view(np.uint32))
            assert np.array_equal(s.column(3).view(np.uint32), right.view(np.uint32))
        s.close()


def test_samples_add_features_foreground_in_the_last_chunk_only(ctx):
    """Three chunks (GATHER_CHUNK = 4096), the first two without a foreground voxel: their counts
    are zero and the whole column comes from behind two chunk boundaries."""
    n = 2 * 4096 + 5
    assert (n + 4095) // 4096 == 3
    rng = np.random.default_rng(52)
    lab = np.full(n, 5, np.uint8)                    # non-zero, but no foreground value
    lab[::3] = 0
    lab[2 * 4096:] = [1, 0, 2, 5, 1]
    feat = rng.normal(0, 3, (1, 1, n, 2)).astype(np.float32)
    s = ctx.samples(2)
    for k in (1, 2):
        s.add_features(0, feat, mask=lab.reshape(1, 1, n), foreground=(1, 2))
        assert s.count(0) == s.count(1) == 3 * k
        for col in range(2):
            assert np.array_equal(s.column(col), np.tile(feat[0, 0, [n - 5, n - 3, n - 1], col], k))
    s.close()


def test_samples_add_features_indexed_second_trip(ife):
    """csrc/stats_capi.inc add_features_typed: gather_indexed_kernel runs at most 4096 workgroups
    of 256 lanes."""
    n_idx = 4096 * 256 + 3
    assert n_idx > 4096 * 256
    rng = np.random.default_rng(53)
    shape = (6, 7, 8)
    feat = rng.normal(0, 3, (8,) + shape).astype(np.float32)
    idx = rng.integers(0, 6 * 7 * 8, n_idx)                     # 336 voxels: every one many times
    with _own_context(ife) as c:
        s = c.samples(8)
        s.add_features(0, feat, indices=idx, layout=ife.PLANAR)
        assert all(s.count(col) == n_idx for col in range(8))
        for col in range(8):
            assert np.array_equal(s.column(col).view(np.uint32), feat[col].ravel()[idx].view(np.uint32)), col
        s.close()


def test_mask_image_f64_second_trip(ife, oracle):
    """csrc/ife_capi.hip ife_mask_image_f64: mask_f64_kernel runs at most 4096 workgroups of 256
    lanes.  The checker is the one of test_mask_image_f64 (tests/test_gpu_parity.py)."""
    n = 4096 * 256 + 3
    assert n > 4096 * 256
    rng = np.random.default_rng(54)
    img = rng.normal(0, 100, n)
    m = rng.random(n) * (rng.random(n) >= 0.4)                  # 40 % exact zeros, fractions elsewhere
    assert (m == 0).any() and (m != 0).any()
    with _own_context(ife) as c:
        got = c.mask_image_f64(img, m, -7.5)
    want = oracle.mask_image_f64(img, m, -7.5)
    assert np.array_equal(want, np.where(m != 0, img, -7.5))
    assert got.tobytes() == want.tobytes()


def _labels012(shape, seed):
    m = np.random.default_rng(seed).integers(0, 3, shape).astype(np.uint8)
    m[: shape[0] // 4] = 0
    return m


# csrc/stats_capi.inc ife_samples_add_image: sample_code_kernel runs at most 32768 workgroups of
# four waves, a wave per row segment of 64 voxels; launch_clamp01: clamp01_kernel at most 8192
# workgroups of 256 lanes.  csrc/stats_kernels.hpp SCAN_CHUNK = 4096 row segments.
@pytest.mark.parametrize("shape", [(365, 360, 4), (132, 128, 132)], ids=["code_kernel", "clamp_kernel"])
def test_samples_add_image_many_segments(ife, oracle, synth, shape):
    """The fused sampling (all foreground) over many scan chunks: columns in raster order."""
    nz, ny, nx = shape
    nseg = (nx + 63) // 64 * ny * nz
    if shape == (365, 360, 4):
        assert nseg == 131400 > 32768 * 4              # sample_code_kernel: a second trip
        assert (nseg + 4095) // 4096 == 33             # chunk_sum / scan_chunks / chunk_scan
    else:
        assert nx % 64 == 4 and nseg == 50688          # a ragged third segment per row
        assert (nseg + 4095) // 4096 == 13
        assert nz * ny * nx > 8192 * 256               # clamp01_kernel: a second trip
    img = synth.volume_f32(shape, 57)
    lab = _labels012(shape, 58)
    clamped = np.minimum(lab, 1).astype(np.uint8)
    f = oracle.emphysema_features(img, clamped, 1.0)
    want = oracle.gather_foreground(f, lab, (1, 2))
    with _own_context(ife) as c:
        s = c.samples(8)
        s.add_image(img, lab, [1.0], foreground=(1, 2))
        assert all(s.count(col) == want.shape[1] == int(np.isin(lab, (1, 2)).sum()) for col in range(8))
        got = [s.column(col) for col in range(8)]
        s.close()
    lam1 = np.maximum(np.abs(want[2]).astype(np.float64), 1e-30)
    for col in range(8):
        if col < 2:
            assert np.array_equal(got[col], want[col]), col
        else:   # the bar of test_samples_add_image_u16_labels_and_spacing (tests/test_gpu_stats.py)
            lam = lam1 ** (3 if col == 6 else 1)
            assert (np.abs(got[col].astype(np.float64) - want[col]) / lam).max() <= 3e-6, col


# csrc/dense_capi.inc dense_centres: the same three scan kernels over the row segments' centre counts
@pytest.mark.parametrize("shape,nchunks", [((70, 64, 8), 2), ((365, 360, 4), 33)])
def test_dense_rois_many_segments(ctx, shape, nchunks):
    nz, ny, nx = shape
    nseg = (nx + 63) // 64 * ny * nz
    assert nseg > 4096 and (nseg + 4095) // 4096 == nchunks
    gen = (np.random.default_rng(59).random(shape) < 0.3).astype(np.uint8)
    size = (3, 3, 3)
    want = dense_boxes(gen, size)
    assert len(want) > 4096
    assert ctx._dense_count(gen, size) == len(want)              # the count-only call
    got = ctx.dense_rois(gen, size)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
