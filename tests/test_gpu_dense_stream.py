"""The dense bag as a stream of row blocks (ife_bag_dense_stream_begin / _next / _end): whatever
the blocking, the blocks put together are the bag of ife_bag_image_dense on the same context bit
for bit, and the frequencies are those DenseHistogram::getFrequencies forms from these counts
(int sum, float division, NaN for an empty histogram).

Blockings of the base case (14 x 12 x 70 voxels, box 5 x 3 x 4, two scales, 5 bins: rows of 320
bytes, 600 centres in each of the ten centre planes that have any):
  one block        block_mb = 0 with the default budget
  one plane each   IFE_OPT_DENSE_SCRATCH_MB = 1: the bound taken from the budget, an eighth of what
                   the features and the codes leave of it, is 59 042 bytes = 184 rows < one plane
  three planes     IFE_OPT_DENSE_SCRATCH_MB = 6: the same eighth is 667 362 bytes = 2085 rows,
                   1800 <= 2085 < 2400 (block_mb itself counts whole MiB: 3276 rows, five planes)
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "image-feature-extraction_amd", "host")
BIN = os.path.join(HOST, "bin")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niftiio  # noqa: E402

SIGMAS = [1.0, 2.0]
NBINS = 5
BLOCKINGS = {"one block": 0, "one plane": 1, "three planes": 6}      # name -> IFE_OPT_DENSE_SCRATCH_MB


def centre_plane_counts(gen, size):
    """Centres per z plane by DenseROIGenerator's rule (planes without a fitting box included)."""
    sx, sy, sz = size
    nz, ny, nx = gen.shape
    fits = np.zeros(gen.shape, bool)
    fits[sz // 2: sz // 2 + nz - sz + 1, sy // 2: sy // 2 + ny - sy + 1, sx // 2: sx // 2 + nx - sx + 1] = True
    return ((gen != 0) & fits).sum(axis=(1, 2))


def device_edges(ctx, img, lab, sigmas, nbins):
    """Equalizing edges of the device's own features over the foreground, one row per column."""
    clamped = np.minimum(lab, 1).astype(np.uint8)
    feats = ctx.emphysema_features(img, clamped, sigmas)
    return np.stack([ctx.equalized_edges(ctx.sort_f32(f[..., c][clamped != 0]), nbins)
                     for f in feats for c in range(8)])


def make_case(ctx, synth, shape, size, seed, base=False, nbins=NBINS):
    nz, ny, nx = shape
    img = synth.volume_f32(shape, seed)
    lab = np.ones(shape, np.uint16)
    lab[:, :, nx // 3:] = 3                      # values above 1
    lab[3:6, 2:5, 1:3] = 0                       # a hole
    lab[nz // 2] = 0                             # an all-zero plane in the middle
    gen = np.ones(shape, np.uint16) * 7
    if base:
        lab[:, :, 58:] = 0                       # boxes around x >= 60 hold no mask voxel
        lab[3:6, 4:8, 20:30] = 0
        gen[:, :, ::11] = 0                      # 60 of the 660 fitting centres of a plane
        gen[6] = 0                               # a centre plane without a centre
    edges = device_edges(ctx, img, lab, SIGMAS, nbins)
    return dict(img=img, lab=lab, gen=gen, size=size, edges=edges)


@pytest.fixture(scope="module")
def base(ctx, synth):
    case = make_case(ctx, synth, (14, 12, 70), (5, 3, 4), 501, base=True)
    case["counts"] = ctx.bag_image_dense(case["img"], case["lab"], SIGMAS, case["size"], case["edges"],
                                         gen_mask=case["gen"])
    case["planes"] = centre_plane_counts(case["gen"], case["size"])
    assert case["counts"].shape == (int(case["planes"].sum()), 16, NBINS)
    assert [int(v) for v in case["planes"]] == [0, 0, 600, 600, 600, 600, 0, 600, 600, 600, 600, 600, 600, 0]
    return case


def stream(ctx, ife, case, values, scratch_mb, gen="case", block_mb=0):
    ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, scratch_mb)
    try:
        return list(ctx.bag_image_dense_stream(case["img"], case["lab"], SIGMAS, case["size"], case["edges"],
                                               gen_mask=case["gen"] if gen == "case" else gen, values=values,
                                               block_mb=block_mb))
    finally:
        ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, 0)


def joined(blocks, n_rois):
    """The blocks are in order, contiguous and non-empty and cover [0, n_rois); their rows."""
    row = 0
    for row0, rows in blocks:
        assert row0 == row and len(rows) > 0
        row += len(rows)
    assert row == n_rois
    return np.concatenate([rows for _, rows in blocks]) if blocks else None


def expected_block_rows(planes, blocking):
    with_centres = [int(v) for v in planes if v > 0]
    per = {"one block": len(with_centres), "one plane": 1, "three planes": 3}[blocking]
    return [sum(with_centres[i:i + per]) for i in range(0, len(with_centres), per)]


def frequencies(counts):
    s = counts.sum(-1, dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(counts) / np.float32(s)[..., None], s


def assert_frequencies(got, counts):
    want, s = frequencies(counts)
    assert got.dtype == np.float32 and got.shape == want.shape
    full = s != 0
    assert np.array_equal(got[full].view(np.uint32), want[full].view(np.uint32))
    assert np.isnan(got[~full]).all() and not np.isnan(got[full]).any()


# ---- 1. counts across blockings ------------------------------------------------------------------
@pytest.mark.parametrize("blocking", list(BLOCKINGS))
def test_counts_are_those_of_the_whole_bag_call(ctx, ife, base, blocking):
    blocks = stream(ctx, ife, base, "counts", BLOCKINGS[blocking])
    assert [len(rows) for _, rows in blocks] == expected_block_rows(base["planes"], blocking)
    if blocking == "three planes":
        assert (base["planes"] > 0).sum() % 3 != 0 and len(base["planes"]) - 4 + 1 == 11
    got = joined(blocks, len(base["counts"]))
    assert got.dtype == np.uint32 and np.array_equal(got, base["counts"])


# ---- 2. frequencies ----------------------------------------------------------------------------------
@pytest.mark.parametrize("blocking", list(BLOCKINGS))
def test_frequencies_are_getfrequencies_of_the_counts(ctx, ife, base, blocking):
    blocks = stream(ctx, ife, base, "frequencies", BLOCKINGS[blocking])
    assert [len(rows) for _, rows in blocks] == expected_block_rows(base["planes"], blocking)
    empty = base["counts"].sum(-1, dtype=np.int32) == 0
    assert empty.all(axis=1).any() and not empty.all()          # rows whose box holds no mask voxel
    assert_frequencies(joined(blocks, len(base["counts"])), base["counts"])


# ---- 3. layouts and degenerate cases -------------------------------------------------------------------
def raw_begin(ctx, ife, img_ptr, lab_ptr, gen_ptr, shape, size, edges, values, block_mb, mem):
    lib = ife.load_library()
    d = ife._desc(shape, (1.0, 1.0, 1.0))
    sig = (C.c_float * len(SIGMAS))(*SIGMAS)
    n, cap = C.c_int64(-1), C.c_int64(-1)
    rc = lib.ife_bag_dense_stream_begin(ctx._h, img_ptr, ife.F32, lab_ptr, ife.U16, gen_ptr, ife.U16, C.byref(d),
                                        sig, len(SIGMAS), (C.c_int64 * 3)(*size), edges.ctypes.data,
                                        edges.shape[1], values, block_mb, C.byref(n), C.byref(cap), mem)
    return rc, n.value, cap.value


def raw_next(ctx, ife, buf, capacity=None):
    row0, n = C.c_int64(-1), C.c_int64(-1)
    rc = ife.load_library().ife_bag_dense_stream_next(ctx._h, buf.ctypes.data if buf is not None else None,
                                                      len(buf) if capacity is None else capacity,
                                                      C.byref(row0), C.byref(n))
    return rc, row0.value, n.value


def raw_drain(ctx, ife, cap, dtype, between=None):
    blocks = []
    while True:
        buf = np.empty((max(cap, 1), 16, NBINS), dtype)
        rc, row0, n = raw_next(ctx, ife, buf)
        assert rc == ife.OK, ife.load_library().ife_last_error(ctx._h)
        if n == 0:
            return blocks
        blocks.append((row0, buf[:n]))
        if between:
            between()


def test_inputs_in_device_memory(ctx, ife, base):
    import torch
    dev = [torch.from_numpy(a).cuda() for a in (base["img"], base["lab"].view(np.int16), base["gen"].view(np.int16))]
    torch.cuda.synchronize()
    ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, 6)
    try:
        rc, n, cap = raw_begin(ctx, ife, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), base["img"].shape,
                               base["size"], base["edges"], ife.BAG_FREQUENCIES, 0, ife.MEM_DEVICE)
        assert rc == ife.OK and n == len(base["counts"]) and cap == 1800
        blocks = raw_drain(ctx, ife, cap, np.float32)
    finally:
        ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, 0)
        assert ife.load_library().ife_bag_dense_stream_end(ctx._h) == ife.OK
    assert len(blocks) == 4
    assert_frequencies(joined(blocks, n), base["counts"])


def test_the_mask_generates_when_no_generating_mask_is_given(ctx, ife, base):
    want = ctx.bag_image_dense(base["img"], base["lab"], SIGMAS, base["size"], base["edges"])
    assert 0 < len(want) != len(base["counts"])
    blocks = stream(ctx, ife, base, "counts", 1, gen=None)
    assert len(blocks) > 1
    assert np.array_equal(joined(blocks, len(want)), want)


def test_box_larger_than_the_volume_is_an_empty_stream(ctx, ife, base):
    assert stream(ctx, ife, dict(base, size=(5, 13, 4)), "frequencies", 0) == []
    rc, n, cap = raw_begin(ctx, ife, base["img"].ctypes.data, base["lab"].ctypes.data, None, base["img"].shape,
                           (71, 3, 4), base["edges"], ife.BAG_COUNTS, 0, ife.MEM_HOST)
    assert (rc, n, cap) == (ife.OK, 0, 0)
    assert raw_next(ctx, ife, np.empty((1, 16, NBINS), np.uint32)) == (ife.OK, 0, 0)   # the first _next ends it
    assert ife.load_library().ife_bag_dense_stream_end(ctx._h) == ife.OK


@pytest.mark.parametrize("shape,size", [((8, 6, 64), (5, 3, 4)), ((8, 6, 5), (5, 3, 4))])
def test_one_full_segment_and_a_single_centre_column(ctx, ife, synth, shape, size):
    case = make_case(ctx, synth, shape, size, 503)
    want = ctx.bag_image_dense(case["img"], case["lab"], SIGMAS, size, case["edges"], gen_mask=case["gen"])
    planes = centre_plane_counts(case["gen"], size)
    assert len(want) == planes.sum() == 5 * 4 * (shape[2] - 4)
    for scratch_mb in (0, 1):
        blocks = stream(ctx, ife, case, "counts", scratch_mb)
        assert np.array_equal(joined(blocks, len(want)), want)
        assert_frequencies(joined(stream(ctx, ife, case, "frequencies", scratch_mb), len(want)), want)
    if shape[2] == 64:
        assert len(blocks) == 5                  # 240 rows a plane, the bound from 1 MiB is below two planes


# ---- 4. protocol -------------------------------------------------------------------------------------------
def test_next_and_end_need_a_begin(ife):
    with ife.Context(0) as fresh:
        rc, _, _ = raw_next(fresh, ife, np.empty((1, 16, NBINS), np.uint32))
        assert rc == ife.E_STATE and ife.load_library().ife_last_error(fresh._h)
        assert ife.load_library().ife_bag_dense_stream_end(fresh._h) == ife.E_STATE


def begin_base(ctx, ife, base, values, scratch_mb):
    ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, scratch_mb)
    try:
        rc, n, cap = raw_begin(ctx, ife, base["img"].ctypes.data, base["lab"].ctypes.data, base["gen"].ctypes.data,
                               base["img"].shape, base["size"], base["edges"], values, 0, ife.MEM_HOST)
    finally:
        ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, 0)
    assert rc == ife.OK and n == len(base["counts"])
    return cap


def test_a_small_array_is_refused_and_the_block_comes_on_retry(ctx, ife, base):
    lib = ife.load_library()
    cap = begin_base(ctx, ife, base, ife.BAG_COUNTS, 6)
    assert cap == 1800
    first = np.empty((cap, 16, NBINS), np.uint32)
    assert raw_next(ctx, ife, first) == (ife.OK, 0, 1800)
    small = np.full((1799, 16, NBINS), 0xdeadbeef, np.uint32)
    assert raw_next(ctx, ife, small) == (ife.E_SIZE, 1800, 1800)     # the rows are reported
    assert np.all(small == 0xdeadbeef) and lib.ife_last_error(ctx._h)
    assert raw_next(ctx, ife, small, capacity=0) == (ife.E_SIZE, 1800, 1800)
    second = np.empty((cap, 16, NBINS), np.uint32)
    assert raw_next(ctx, ife, second) == (ife.OK, 1800, 1800)        # nothing was consumed
    rest = raw_drain(ctx, ife, cap, np.uint32)
    assert lib.ife_bag_dense_stream_end(ctx._h) == ife.OK
    assert lib.ife_bag_dense_stream_end(ctx._h) == ife.E_STATE
    got = joined([(0, first), (1800, second)] + rest, len(base["counts"]))
    assert np.array_equal(got, base["counts"])


def test_other_calls_between_the_blocks_do_not_disturb_the_stream(ctx, ife, base):
    rng = np.random.default_rng(71)
    shape, size = (18, 22, 26), (7, 5, 6)
    feat = np.round(rng.normal(0, 3, shape + (8,)), 1).astype(np.float32)
    m = rng.integers(0, 3, shape).astype(np.uint8)
    edges = np.sort(np.round(rng.normal(0, 3, (8, 13)), 1).astype(np.float32), axis=1)
    want_other = ctx.dense_roi_histograms(feat, m, size, edges)
    others = []
    cap = begin_base(ctx, ife, base, ife.BAG_FREQUENCIES, 1)
    blocks = raw_drain(ctx, ife, cap, np.float32,
                       between=lambda: others.append(ctx.dense_roi_histograms(feat, m, size, edges)))
    assert ife.load_library().ife_bag_dense_stream_end(ctx._h) == ife.OK
    assert len(blocks) == 10 == len(others)
    assert_frequencies(joined(blocks, len(base["counts"])), base["counts"])
    assert all(np.array_equal(o, want_other) for o in others)


def test_a_second_begin_without_end_starts_cleanly(ctx, ife, base):
    cap = begin_base(ctx, ife, base, ife.BAG_COUNTS, 1)
    buf = np.empty((cap, 16, NBINS), np.uint32)
    assert raw_next(ctx, ife, buf) == (ife.OK, 0, 600)
    assert raw_next(ctx, ife, buf) == (ife.OK, 600, 600)
    cap = begin_base(ctx, ife, base, ife.BAG_COUNTS, 6)              # the first stream is dropped
    blocks = raw_drain(ctx, ife, cap, np.uint32)
    assert ife.load_library().ife_bag_dense_stream_end(ctx._h) == ife.OK
    assert [r for r, _ in blocks] == [0, 1800, 3600, 5400]
    assert np.array_equal(joined(blocks, len(base["counts"])), base["counts"])
    # a generator left early ends its stream
    it = ctx.bag_image_dense_stream(base["img"], base["lab"], SIGMAS, base["size"], base["edges"],
                                    gen_mask=base["gen"], values="counts")
    row0, rows = next(it)
    it.close()
    assert row0 == 0 and np.array_equal(rows, base["counts"])
    assert ife.load_library().ife_bag_dense_stream_end(ctx._h) == ife.E_STATE


# ---- 5. the transposition at every tile shape --------------------------------------------------------------
# csrc/dense_capi.inc dense_stream_count: dense_freq_kernel stages 64 rows x `hists` whole histograms
# in DENSE_FREQ_LDS_WORDS = 12288 words of LDS at a pitch of rows + 1, 32 rows where one histogram
# does not fit beside 64 (nb * 65 > 12288, that is nb >= 190); the last group of histograms and
# the last tile of rows are partial where nothing divides.
# Not reached: the strided y grid.  It needs more than 65535 groups of histograms, that is more
# than 8192 scales.
FREQ_LDS_WORDS = 12288
NCOL = 8 * len(SIGMAS)
# bins: rows of a tile, histograms of a group, groups, histograms of the last group
TILINGS = {30: (64, 6, 3, 4), 189: (64, 1, 16, 1), 190: (32, 1, 16, 1), 255: (32, 1, 16, 1)}


def tiling(nb, ncol):
    tr = 64 if nb * 65 <= FREQ_LDS_WORDS else 32
    hists = max(1, min(ncol, FREQ_LDS_WORDS // (tr + 1) // nb))
    groups = -(-ncol // hists)
    return tr, hists, groups, ncol - (groups - 1) * hists


@pytest.fixture(scope="module", params=sorted(TILINGS))
def many_bins(request, ctx, synth):
    """The base case with `nb` bins and the bag ife_bag_image_dense gives for it: once per bin count,
    shared by the four streams, never written to."""
    nb = request.param
    case = make_case(ctx, synth, (14, 12, 70), (5, 3, 4), 501, base=True, nbins=nb)
    assert case["edges"].shape == (NCOL, nb - 1)
    case["nb"] = nb
    case["counts"] = ctx.bag_image_dense(case["img"], case["lab"], SIGMAS, case["size"], case["edges"],
                                         gen_mask=case["gen"])
    assert case["counts"].shape == (6000, NCOL, nb)
    for a in (case["img"], case["lab"], case["gen"], case["edges"], case["counts"]):
        a.setflags(write=False)
    return case


@pytest.mark.parametrize("block_mb", [0, 1], ids=["one-block", "one-plane"])
@pytest.mark.parametrize("values", ["counts", "frequencies"])
def test_transposition_at_every_tile_shape(ctx, ife, many_bins, values, block_mb):
    nb = many_bins["nb"]
    tr, hists, groups, last = tiling(nb, NCOL)
    assert (tr, hists, groups, last) == TILINGS[nb]
    if nb == 30:
        assert 0 < last < hists                          # a partial last group of histograms
    if nb == 189:
        assert tiling(nb + 1, NCOL)[0] == 32             # the last bin count with 64-row tiles
    blocks = stream(ctx, ife, many_bins, values, 0, block_mb=block_mb)
    rows = [len(r) for _, r in blocks]
    if block_mb:                                         # the 600 rows of one plane are beyond 1 MiB already
        assert 600 * NCOL * nb * 4 > 1 << 20
        assert rows == [600] * 10
    else:
        assert rows == [6000]
    assert all(n % tr != 0 for n in rows)                # the last tile of rows is partial
    got = joined(blocks, 6000)
    if values == "counts":
        assert got.dtype == np.uint32 and np.array_equal(got, many_bins["counts"])
    else:
        empty = many_bins["counts"].sum(-1, dtype=np.int32) == 0
        assert empty.any() and not empty.all()
        assert_frequencies(got, many_bins["counts"])


# ---- 6. the tool ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "image-feature-extraction_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return BIN


def test_makebag_dense_streams_the_same_bag(built, tmp_path, synth, oracle):
    """tests/test_host_tools_dense.py at its shape, with two scales and 255 bins: a row is 16 320
    bytes, the 55 regions of a centre plane 897 600, so IFE_DENSE_BLOCK_MB=1 gives one plane per
    block, three blocks."""
    shape, nbins, scales = (10, 12, 14), 255, (1.0, 2.0)
    sx, sy, sz = 4, 3, 2
    img = synth.volume_f32(shape, 403)
    lab = np.zeros(shape, np.uint16)
    lab[2:8, 2:10, 3:12] = 2
    roi_mask = np.zeros(shape, np.uint16)
    roi_mask[1:9, 1:11, 1:13] = 3
    roi_mask[3:6, 4:9, 2:14] = 5                       # reaches outside the image mask and to the x border
    roi_mask[0, 0, 0] = 5                              # a voxel whose box does not fit
    niftiio.write(str(tmp_path / "img.nii.gz"), img)
    niftiio.write(str(tmp_path / "lab.nii.gz"), lab)
    niftiio.write(str(tmp_path / "roi.nii.gz"), roi_mask)
    clamped = np.minimum(lab, 1).astype(np.uint8)
    feats = [oracle.emphysema_features(img, clamped, s) for s in scales]
    edges = np.stack([oracle.equalized_edges(oracle.sort_f32(f[..., c][clamped != 0]), nbins)
                      for f in feats for c in range(8)])
    edges32 = np.array([[np.float32(float("%.9g" % v)) for v in row] for row in edges], np.float32)
    (tmp_path / "hist.txt").write_text("".join(",".join("%.9g" % v for v in row) + "\n" for row in edges))
    outputs = {}
    for name, env in (("stream", {"IFE_DENSE_BLOCK_MB": "1"}), ("whole", {"IFE_DENSE_STREAM": "0"})):
        os.mkdir(str(tmp_path / name))
        r = subprocess.run([os.path.join(BIN, "MakeBagDense"), "-i", str(tmp_path / "img.nii.gz"),
                            "-m", str(tmp_path / "lab.nii.gz"), "-M", str(tmp_path / "roi.nii.gz"), "-v", "5",
                            "-H", str(tmp_path / "hist.txt"), "-o", str(tmp_path / name), "-s", "1", "-s", "2",
                            "-x", str(sx), "-y", str(sy), "-z", str(sz), "-p", "dense"],
                           capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr
        outputs[name] = ((tmp_path / name / "dense.bag").read_text().replace("-nan", "nan"),
                         (tmp_path / name / "dense.ROIInfo").read_text())
    assert outputs["stream"] == outputs["whole"]
    want_boxes = []
    for z, y, x in zip(*np.nonzero(roi_mask == 5)):    # np.nonzero walks z, y, x: raster order
        x0, y0, z0 = x - sx // 2, y - sy // 2, z - sz // 2
        if x0 >= 0 and y0 >= 0 and z0 >= 0 and x0 + sx <= 14 and y0 + sy <= 12 and z0 + sz <= 10:
            want_boxes.append((x0, y0, z0, sx, sy, sz))
    assert len(want_boxes) == 3 * 55
    assert outputs["stream"][1].splitlines() == ["[%d, %d, %d][%d, %d, %d]" % b for b in want_boxes]
    rows = outputs["stream"][0].splitlines()
    assert len(rows) == len(want_boxes)
    boxes = np.array(want_boxes, np.int64)
    fr = np.concatenate([oracle.roi_histograms(f, clamped, boxes, edges32[i * 8:(i + 1) * 8])[1]
                         for i, f in enumerate(feats)], axis=1)
    for j, row in enumerate(rows):
        assert row.split(",") == ["%g" % v for v in fr[j].ravel()], j
