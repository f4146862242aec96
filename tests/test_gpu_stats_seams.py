"""The statistics kernels (csrc/stats_kernels.hpp, csrc/stats_capi.inc) where their structure has
seams: the radix sort at tile and scan-segment boundaries, as a batch of columns with a stride that
is not the count, on digit distributions that random floats never produce and over groups of
columns of unequal counts; the edge walk's status 3 and the batched edges; the per-box histogram
at its z split and LDS limit; the dense histogram at its edge limit and on ties, infinities and a
NaN.  The checker is tests/stats_oracle.py (held to the oracle by tests/test_stats_oracle_cpu.py);
a sort is compared bit for bit in the order of `f32_to_key`, which puts -0 before +0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stats_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

T = 16384   # SORT_TILE, asserted against the header in test_sort_seams


def fill(s, c, col):
    """Append col to column c of a Samples object."""
    col = np.ascontiguousarray(col, np.float32)
    s.add_features(c, col.reshape(1, 1, -1, 1), indices=np.arange(col.size))


def samples_with(ctx, cols, spare=0):
    """One column per entry of cols (an empty entry stays empty).  spare > 0: a longer column is
    added and cleared first, so the capacity, which is the stride between columns, exceeds every count."""
    s = ctx.samples(len(cols))
    if spare:
        fill(s, 0, np.zeros(max(len(c) for c in cols) + spare, np.float32))
        s.clear()
        assert all(s.count(c) == 0 for c in range(len(cols)))
    for c, col in enumerate(cols):
        if len(col):
            fill(s, c, col)
    return s


def assert_columns_sorted(s, cols):
    for c, col in enumerate(cols):
        assert s.count(c) == len(col), c
        if len(col):
            assert so.same_bits(s.column(c), so.sorted_bits(col)), c


# ---- 3. sort: seams and batches -----------------------------------------------------------------
SEAMS = [(16383, 1, 1), (16384, 1, 1), (16385, 2, 1), (16 * 16384, 16, 1), (16 * 16384 + 1, 17, 2),
         (31 * 16384 - 5, 31, 2), (33 * 16384 - 5, 33, 3)]


@pytest.mark.parametrize("n,ntiles,seg_tiles", SEAMS)
def test_sort_seams(ctx, n, ntiles, seg_tiles):
    k = so.kernel_constants()
    tile = k["SORT_THREADS"] * k["SORT_KPT"] * k["SORT_SUB"]
    assert tile == T == so.SORT_TILE and k["SORT_SEGS"] == so.SORT_SEGS == 16
    nt = -(-n // tile)
    assert (nt, -(-nt // k["SORT_SEGS"])) == (ntiles, seg_tiles) == so.sort_geometry(n)
    if ntiles == 17:   # the last used segment holds one tile of one key, seven segments hold none
        used = -(-ntiles // seg_tiles)
        assert used == 9 and ntiles - (used - 1) * seg_tiles == 1 and n - (ntiles - 1) * tile == 1
    v = so.mixed_column(n, n)
    assert so.same_bits(ctx.sort_f32(v), so.sorted_bits(v))


@pytest.mark.parametrize("n", [16385, 16 * 16384 + 1, 33 * 16384 - 5])
def test_sort_batches(ctx, n):
    """Three columns in one launch (blockIdx.y), table and segment sums per column, stride > n."""
    cols = [so.mixed_column(n, 100 + n, 1000.0),
            so.sorted_bits(so.mixed_column(n, 200 + n, 3.0)),                  # presorted
            so.sorted_bits(so.mixed_column(n, 300 + n, 1e-3))[::-1].copy()]    # reversed
    assert not so.same_bits(cols[0], cols[1]) and not so.same_bits(cols[1], cols[2][::-1].copy())
    s = samples_with(ctx, cols, spare=1000)
    s.sort()
    assert_columns_sorted(s, cols)
    s.close()


DIGIT_N = 16384 + 4096 + 70   # a ragged second tile whose last sub-tile has 70 keys: one full round
                              # of wave 0, then a round with 6 valid lanes


def _with_byte(base, b, values):
    base = np.asarray(base, np.uint32)
    return (base & np.uint32(~(0xFF << (8 * b)) & 0xFFFFFFFF)) | (np.asarray(values, np.uint32) << np.uint32(8 * b))


def one_byte_columns(rng):
    """Column b: keys that differ in byte b only; the other three passes see one digit."""
    cols = []
    for b in range(4):
        lo, hi = (1, 255) if b == 3 else (0, 256)   # keys 0x00...... and 0xff...... are mostly NaNs
        cols.append(so.from_keys(_with_byte(np.full(DIGIT_N, 0xC0804020, np.uint32), b,
                                            rng.integers(lo, hi, DIGIT_N))))
    return cols


def alternating_columns(rng):
    """Column b: byte b alternates between two digits by position, the other bytes are random, so the
    ranking of pass b sees two interleaved ballots and must stay stable over what the lower passes did."""
    cols = []
    for b in range(4):
        k = rng.integers(0, 1 << 32, DIGIT_N, dtype=np.uint64).astype(np.uint32)
        k = _with_byte(k, 3, rng.integers(1, 255, DIGIT_N))
        pair = (0x40, 0xBF) if b == 3 else (0x00, 0xFF)
        cols.append(so.from_keys(_with_byte(k, b, np.where(np.arange(DIGIT_N) % 2 == 0, *pair))))
    return cols


def extreme_columns(rng):
    """FLT_MAX (key 0xff7fffff: digit 255 in passes 0, 1 and 3) and +inf (0xff800000) with a few
    ordinary values, so that valid keys of digit 255 sit next to the 0xffffffff of the padding
    lanes; the mirror of -FLT_MAX and -inf (digit 0) with denormals of both signs and both zeros;
    and both again in their hardest order for a stable pass, descending."""
    fmax = np.float32(3.4028235e38)
    hi = np.where(rng.random(DIGIT_N) < 0.6, fmax, np.float32(np.inf)).astype(np.float32)
    hi[rng.permutation(DIGIT_N)[:40]] = rng.normal(0, 1, 40).astype(np.float32)
    hi[-70:] = fmax                                  # the ragged sub-tile of pass 0 is all digit 255
    lo = np.where(rng.random(DIGIT_N) < 0.6, -fmax, np.float32(-np.inf)).astype(np.float32)
    small = np.array([1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 0.0, -0.0], np.float32)
    lo[rng.permutation(DIGIT_N)[:600]] = np.resize(small, 600)
    lo[-70:] = -fmax
    assert so.keys(hi[-1:])[0] == 0xFF7FFFFF and so.keys(np.array([np.inf], np.float32))[0] == 0xFF800000
    assert so.keys(lo[-1:])[0] == 0x00800000 and so.keys(np.array([-np.inf], np.float32))[0] == 0x007FFFFF
    return [hi, lo, so.sorted_bits(hi)[::-1].copy(), so.sorted_bits(lo)[::-1].copy()]


@pytest.mark.parametrize("make", [one_byte_columns, alternating_columns, extreme_columns])
def test_sort_digit_distributions(ctx, make):
    assert so.SORT_SUBTILE == 4096 and DIGIT_N - T - 4096 == 70 == 64 + 6
    cols = make(np.random.default_rng(77))
    assert len(cols) == 4 and all(c.size == DIGIT_N for c in cols)
    s = samples_with(ctx, cols, spare=333)
    s.sort()
    assert_columns_sorted(s, cols)
    s.close()
    for c in cols[:2]:                                # the single-column entry takes the same passes
        assert so.same_bits(ctx.sort_f32(c), so.sorted_bits(c))


def test_sort_groups_of_unequal_counts(ctx):
    """Groups (0,1) (2) (3) (4) (5) (6,7): data and tmp are offset by group, a column of no and of
    one sample is left alone, a column of 5 is one ragged round."""
    counts = [20000, 20000, 5, 0, 1, 20000, 16385, 16385]
    cols = [so.mixed_column(n, 400 + c, 10.0 ** (c - 3)) if n else np.zeros(0, np.float32)
            for c, n in enumerate(counts)]
    s = samples_with(ctx, cols)
    for c, col in enumerate(cols):                    # as added: raster order
        assert s.count(c) == counts[c]
        if counts[c]:
            assert so.same_bits(s.column(c), col), c
    s.sort()
    assert_columns_sorted(s, cols)
    s.sort()                                          # sorted already: nothing moves
    assert_columns_sorted(s, cols)
    more = np.array([-np.inf, 0.5, np.inf], np.float32)
    fill(s, 2, more)                                  # re-sorts every (sorted) column
    cols[2] = np.concatenate([so.sorted_bits(cols[2]), more])
    s.sort()
    assert_columns_sorted(s, cols)
    assert s.count(3) == 0
    s.close()


# ---- 4. edges -----------------------------------------------------------------------------------
def test_edges_status_3_on_purpose(ctx, ife, oracle):
    for dt in (np.float32, np.float64):
        v = np.array(so.RC3_VALUES, dt)
        assert so.walk(v, so.RC3_BINS)[0] == 3
        with pytest.raises(oracle.EdgeWalkError) as eo:
            oracle.equalized_edges(v, so.RC3_BINS)
        assert eo.value.rc == 3
        with pytest.raises(ife.IfeError) as ei:
            ctx.equalized_edges(v, so.RC3_BINS)
        assert ei.value.code == ife.E_STATE and "ran past the last sample" in str(ei.value)
    assert ctx.equalized_edges(np.array(so.RC3_VALUES, np.float32), 2).tolist() == [1.0]   # still usable


EDGE_A, EDGE_B = 20000, 4999


@pytest.mark.parametrize("nbins", [2, 5, 9])
def test_batched_edges_unequal_counts(ctx, oracle, nbins):
    """Counts (A, A, B, B, A): three groups, the edges and status rows offset by group."""
    rng = np.random.default_rng(81)
    cols = [np.round(rng.normal(0, 1 + c, n) * 3).astype(np.float32)
            for c, n in enumerate([EDGE_A, EDGE_A, EDGE_B, EDGE_B, EDGE_A])]
    s = samples_with(ctx, cols, spare=77)
    got = s.equalized_edges(nbins)
    assert got.shape == (5, nbins - 1)
    for c, col in enumerate(cols):
        want = oracle.equalized_edges(so.sorted_bits(col), nbins)
        assert so.same_bits(got[c], want), c
        assert so.walk(so.sorted_bits(col), nbins)[0] == 0
    assert_columns_sorted(s, cols)
    s.close()


def test_batched_edges_errors_name_the_column(ctx, ife):
    ramp = lambda n, k: np.arange(n, dtype=np.float32) * k  # noqa: E731
    cols = [ramp(10, 1), ramp(10, 2), ramp(7, 3), np.array(so.RC3_VALUES, np.float32), ramp(7, 5)]
    s = samples_with(ctx, cols)
    with pytest.raises(ife.IfeError) as ei:
        s.equalized_edges(so.RC3_BINS)
    assert ei.value.code == ife.E_STATE and "column 3:" in str(ei.value), str(ei.value)
    want = np.stack([so.walk(c, 2)[1] for c in cols])             # two bins walk through everywhere
    assert so.same_bits(s.equalized_edges(2), want)
    s.close()
    cols[3], cols[2] = ramp(7, 7), ramp(2, 3)                      # column 2: 2 samples for 3 bins
    s = samples_with(ctx, cols)
    with pytest.raises(ife.IfeError) as ei:
        s.equalized_edges(3)
    assert ei.value.code == ife.E_ARG and "Too many bins" in str(ei.value) and "column 2:" in str(ei.value)
    s.close()


@pytest.mark.parametrize("distinct", [3, 1000])
def test_edges_long_walk_few_distinct_values(ctx, ife, oracle, distinct):
    n = 200001
    v32 = np.sort(np.random.default_rng(distinct).integers(0, distinct, n)).astype(np.float32)
    assert np.unique(v32).size == distinct
    for nbins in (2, 64, 1000):
        for v in (v32, v32.astype(np.float64)):
            try:
                want = oracle.equalized_edges(v, nbins)
            except oracle.EdgeWalkError as e:
                assert so.walk(v, nbins)[0] == e.rc
                with pytest.raises(ife.IfeError) as ei:
                    ctx.equalized_edges(v, nbins)
                assert ei.value.code == (ife.E_ARG if e.rc == 1 else ife.E_STATE), (nbins, v.dtype)
                continue
            got = ctx.equalized_edges(v, nbins)
            assert got.dtype == v.dtype and np.array_equal(got, want), (nbins, v.dtype)


# ---- 5. roi_histograms --------------------------------------------------------------------------
ROI_SHAPE = (20, 17, 19)


def z_split_boxes():
    nz, ny, nx = ROI_SHAPE
    boxes = []
    for sz in (1, 7, 8, 9, 17):                       # ROI_SPLIT = 8: 1, 1, 1, 2 and 3 planes per workgroup
        for z0 in (0, nz - sz):
            boxes.append([2, 1, z0, 3, 4, sz])        # 12 voxels per plane: one partial round of 256
            boxes.append([0, 0, z0, nx, ny, sz])      # 323 voxels per plane: a plane spans two rounds
    return np.array(boxes, np.int64)


@pytest.mark.parametrize("form", ["interleaved_u8", "interleaved_u16", "planar_u8", "planar_u16"])
@pytest.mark.parametrize("masked", [False, True])
def test_roi_histograms_z_split(ctx, ife, oracle, form, masked):
    assert so.kernel_constants()["ROI_SPLIT"] == so.ROI_SPLIT == 8
    nz, ny, nx = ROI_SHAPE
    feat, edges = so.coordinate_features(ROI_SHAPE), so.coordinate_edges(ROI_SHAPE)
    mask = np.ones(ROI_SHAPE, np.uint8)
    if masked:
        mask = (np.random.default_rng(91).random(ROI_SHAPE) < 0.6).astype(np.uint8) * 3
        mask[[0, 8, 16, 19]] = 0                      # whole planes, the first and the last among them
    rois = z_split_boxes()
    assert 3 * 4 < 256 < nx * ny
    closed = so.coordinate_counts(mask, rois)
    want, _ = oracle.roi_histograms(feat, np.minimum(mask, 1), rois, edges)
    assert np.array_equal(closed, want)
    m = (mask != 0).astype(np.uint16) * 256 if form.endswith("u16") else mask   # label 256: its low byte is 0
    if form.startswith("planar"):
        got = ctx.roi_histograms(np.ascontiguousarray(np.moveaxis(feat, -1, 0)), m, rois, edges, layout=ife.PLANAR)
    else:
        got = ctx.roi_histograms(feat, m, rois, edges)
    for r, (x0, y0, z0, sx, sy, sz) in enumerate(rois):   # every plane of the box once, no other plane
        planes = (mask[:, y0:y0 + sy, x0:x0 + sx] != 0).sum(axis=(1, 2))
        planes[:z0] = 0
        planes[z0 + sz:] = 0
        assert got[r, 2, :nz].tolist() == planes.tolist(), (r, rois[r])
        if not masked:
            assert got[r, 2, z0:z0 + sz].tolist() == [sx * sy] * sz
    assert np.array_equal(got, closed)


def test_roi_histograms_empty_boxes(ctx, oracle):
    feat, edges = so.coordinate_features(ROI_SHAPE), so.coordinate_edges(ROI_SHAPE)
    mask = np.ones(ROI_SHAPE, np.uint8)
    rois = np.array([[1, 2, 3, 4, 5, 9], [1, 2, 3, 0, 5, 9], [5, 5, 5, 6, 7, 8], [1, 2, 3, 4, 0, 9],
                     [1, 2, 3, 4, 5, 0], [19, 17, 20, 0, 0, 0], [0, 0, 11, 19, 17, 9]], np.int64)
    got = ctx.roi_histograms(feat, mask, rois, edges)
    want, _ = oracle.roi_histograms(feat, mask, rois, edges)
    assert np.array_equal(got, want) and np.array_equal(got, so.coordinate_counts(mask, rois))
    for r in (1, 3, 4, 5):
        assert not got[r].any()
    for r in (0, 2, 6):
        assert got[r, 0].sum() == rois[r, 3] * rois[r, 4] * rois[r, 5]


LDS_SHAPE = (6, 7, 8)


@pytest.mark.parametrize("ncomp,ne", [(8, 511), (2, 2047), (1, 4095)])
def test_roi_histograms_at_the_lds_limit(ctx, ife, oracle, ncomp, ne):
    words = ncomp * (2 * ne + 1)
    assert words <= so.ROI_MAX_LDS_WORDS < words + 2 * ncomp      # one more edge per component does not fit
    rng = np.random.default_rng(ne)
    feat = rng.normal(0, 3, LDS_SHAPE + (ncomp,)).astype(np.float32)
    feat[1, 1, 1, 0] = -1e9                                         # first bin of the first component
    feat[4, 5, 6, ncomp - 1] = 1e9                                  # last bin of the last component
    edges = np.sort(rng.normal(0, 3, (ncomp, ne)).astype(np.float32), axis=1)
    mask = np.ones(LDS_SHAPE, np.uint8)
    mask[2, 3] = 0
    rois = [[0, 0, 0, 8, 7, 6], [1, 1, 1, 6, 5, 5]]
    want, _ = oracle.roi_histograms(feat, mask, rois, edges)
    assert want[0, 0, 0] > 0 and want[1, 0, 0] > 0 and want[0, -1, -1] > 0 and want[1, -1, -1] > 0
    got = ctx.roi_histograms(feat, mask, rois, edges)
    assert got.shape == (2, ncomp, ne + 1) and np.array_equal(got, want)
    planar = np.ascontiguousarray(np.moveaxis(feat, -1, 0))
    assert np.array_equal(ctx.roi_histograms(planar, mask, rois, edges, layout=ife.PLANAR), want)


@pytest.mark.parametrize("ncomp,ne", [(8, 512), (2, 2048), (1, 4096)])
def test_roi_histograms_beyond_the_lds_limit_are_refused(ctx, ife, ncomp, ne):
    assert ncomp * (2 * ne + 1) > so.ROI_MAX_LDS_WORDS >= ncomp * (2 * (ne - 1) + 1)
    feat = np.zeros(LDS_SHAPE + (ncomp,), np.float32)
    edges = np.tile(np.arange(ne, dtype=np.float32), (ncomp, 1))
    mask = np.ones(LDS_SHAPE, np.uint8)
    rois = np.array([[0, 0, 0, 8, 7, 6]], np.int64)
    counts = np.full((1, ncomp, ne + 1), 0xA5A5A5A5, np.uint32)
    d = ife.VolumeDesc(8, 7, 6, 1.0, 1.0, 1.0)
    rc = ctx._lib.ife_roi_histograms(ctx._h, feat.ctypes.data, ife.INTERLEAVED, ncomp, mask.ctypes.data, ife.U8,
                                     C.byref(d), rois.ctypes.data, 1, edges.ctypes.data, ne, counts.ctypes.data,
                                     ife.MEM_HOST)
    assert rc == ife.E_ARG
    assert np.all(counts == 0xA5A5A5A5)                             # refused before anything was written
    with pytest.raises(ife.IfeError) as ei:
        ctx.roi_histograms(feat, mask, rois, edges)
    assert ei.value.code == ife.E_ARG and str(so.ROI_MAX_LDS_WORDS) in str(ei.value)


def test_bag_image_refuses_512_edges(ctx, ife, synth):
    shape = (8, 8, 8)
    img = synth.volume_f32(shape, 5)
    mask = np.ones(shape, np.uint8)
    rois = [[0, 0, 0, 4, 4, 4]]
    with pytest.raises(ife.IfeError) as ei:
        ctx.bag_image(img, mask, [1.0], rois, np.tile(np.arange(512, dtype=np.float32), (8, 1)))
    assert ei.value.code == ife.E_ARG and "511" in str(ei.value)
    got = ctx.bag_image(img, mask, [1.0], rois, np.tile(np.arange(511, dtype=np.float32), (8, 1)))
    assert got.shape == (1, 8, 512) and np.all(got.sum(axis=2) == 64)   # 511 edges are taken


# ---- 6. dense_histogram -------------------------------------------------------------------------
def test_dense_histogram_edge_limits(ctx, ife):
    assert so.kernel_constants()["HIST_MAX_EDGES"] == so.HIST_MAX_EDGES == 1024
    rng = np.random.default_rng(61)
    v = rng.normal(0, 3, 100003).astype(np.float32)
    edges = np.sort(rng.normal(0, 3, 1024).astype(np.float32))
    v[0], v[1] = edges[0] - 1, edges[-1] + 1                        # the first and the last of 1025 bins
    got = ctx.dense_histogram(edges, v)
    assert got.shape == (1025,) and got[0] > 0 and got[-1] > 0
    assert np.array_equal(got, so.lower_bound_counts(edges, v))
    for bad in (np.arange(1025, dtype=np.float32), np.zeros(0, np.float32)):
        with pytest.raises(ife.IfeError) as ei:
            ctx.dense_histogram(bad, v)
        assert ei.value.code == ife.E_ARG


def test_dense_histogram_value_edge_cases(ctx, oracle):
    n = 524288 + 3                                                  # 2048 workgroups x 256 lanes, and 3: the grid loops
    rng = np.random.default_rng(62)
    edges = np.sort(rng.normal(0, 3, 300).astype(np.float32))
    edges[100:103] = edges[100]                                     # three equal edges: bins 101 and 102 stay empty
    edges[150] = 0.0                                                # both zeros fall in the bin that ends at 0.0
    edges = np.sort(edges)
    i0 = int(np.searchsorted(edges, 0.0))
    assert edges[i0] == 0.0 and edges[100] == edges[101] == edges[102]
    v = rng.normal(0, 4, n).astype(np.float32)
    v[::7] = edges[rng.integers(0, edges.size, v[::7].size)]       # exact copies of edges
    v[1], v[2], v[3], v[4] = np.inf, -np.inf, 0.0, -0.0
    v[5:12:2] = edges[100]
    v[n - 2] = np.nan
    want = so.lower_bound_counts(edges, v)
    got = ctx.dense_histogram(edges, v)
    assert np.array_equal(got, want)
    assert got.sum() == n and got[101] == 0 and got[102] == 0 and got[100] > 3 and got[-1] >= 1
    clean = v[~np.isnan(v)]
    assert clean.size == n - 1
    c, _ = oracle.dense_histogram(edges, clean)
    assert np.array_equal(ctx.dense_histogram(edges, clean), c)
    assert np.array_equal(got - c, np.eye(1, edges.size + 1, 0, dtype=np.uint32)[0])   # the NaN is in bin 0
    zeros = ctx.dense_histogram(edges, np.array([0.0, -0.0], np.float32))
    assert zeros[i0] == 2 and zeros.sum() == 2


def test_dense_histogram_empty_and_single_bin(ctx):
    edges = np.array([-1.0, 0.0, 2.5], np.float32)
    assert ctx.dense_histogram(edges, np.zeros(0, np.float32)).tolist() == [0, 0, 0, 0]
    n = 300001
    assert ctx.dense_histogram(edges, np.full(n, 2.5, np.float32)).tolist() == [0, 0, n, 0]   # on the edge: (0, 2.5]
    assert ctx.dense_histogram(edges, np.full(n, 7.0, np.float32)).tolist() == [0, 0, 0, n]
    assert ctx.dense_histogram(edges[:1], np.full(n, -1.0, np.float32)).tolist() == [n, 0]
