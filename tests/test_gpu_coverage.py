"""The census and coverage calls on the device (ife_value_census_f32, ife_threshold_mask,
ife_roi_coverage) against tests/coverage_oracle.py, HOST and DEVICE.  Nothing here has a tolerance:
values are compared by their bits, counts for equality.  The shapes are the smallest that reach
every path: the census counts run heads per segment of 256 sorted elements and scans the counts in
chunks of 4096 segments; the coverage planes are words of 32 voxels, formed 256 voxels at a time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_oracle as V  # noqa: E402
import sampling_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu

SEG = 256             # CENSUS_SEG
SCAN_CHUNK = 4096     # segments per chunk of the scan
GUARD = 64
NAN_POS = np.uint32(0x7fc00001).view(np.float32)
NAN_NEG = np.uint32(0xffc00000).view(np.float32)
SHAPE = (3, 5, 37)    # rows of 37 voxels: words straddle rows and planes; 555 voxels, a tail word of 11 bits


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def _device_bytes(torch_dev, payload, offset=0, fill=0xA5):
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


def _guards_intact(t, sl, fill=0xA5):
    h = t.cpu().numpy()
    return (h[:sl.start] == fill).all() and (h[sl.stop:] == fill).all()


# ---- census -------------------------------------------------------------------------------------------
def _census_equal(got, want):
    (u, c, nn), (wu, wc, wn) = got, want
    assert u.dtype == np.float32 and c.dtype == np.uint32
    assert np.array_equal(u.view(np.uint32), wu.view(np.uint32)), (u[:8], wu[:8])
    assert np.array_equal(c, wc) and nn == wn


def _check_census(ctx, torch_dev, values):
    """HOST and DEVICE against the oracle; the DEVICE outputs sit between guards."""
    values = np.ascontiguousarray(values, np.float32)
    want = V.value_census(values)
    _census_equal(ctx.value_census(values), want)
    tv, vptr, _ = _device_bytes(torch_dev, values.tobytes())
    assert ctx.value_census_device(vptr, values.size) == (want[0].size, want[2])      # the counts alone
    cap = want[0].size + 3
    tu, uptr, usl = _device_bytes(torch_dev, bytes([0x5A]) * (4 * cap))
    tc, cptr, csl = _device_bytes(torch_dev, bytes([0x5A]) * (4 * cap))
    assert ctx.value_census_device(vptr, values.size, uptr, cptr, cap) == (want[0].size, want[2])
    u, c = _read(tu, usl, np.float32), _read(tc, csl, np.uint32)
    _census_equal((u[:want[0].size], c[:want[0].size], want[2]), want)
    assert (u[want[0].size:].view(np.uint32) == 0x5A5A5A5A).all() and (c[want[0].size:] == 0x5A5A5A5A).all()
    assert _guards_intact(tu, usl) and _guards_intact(tc, csl)
    assert np.array_equal(_read(tv, slice(GUARD, GUARD + values.nbytes), np.uint32), values.view(np.uint32))
    return want


def test_census_one_element_and_all_equal(ctx, torch_dev):
    assert _check_census(ctx, torch_dev, [3.5])[1][0] == 1
    want = _check_census(ctx, torch_dev, np.full(1000, -2.25, np.float32))
    assert want[0].size == 1 and want[1][0] == 1000


def test_census_all_distinct_and_the_capacity(ife, ctx, torch_dev):
    rng = np.random.default_rng(41)
    n = 777
    values = rng.permutation(n).astype(np.float32) - np.float32(300)
    want = _check_census(ctx, torch_dev, values)
    assert want[0].size == n and (want[1] == 1).all()
    tv, vptr, _ = _device_bytes(torch_dev, values.tobytes())
    for cap in (n, n - 1):
        tu, uptr, usl = _device_bytes(torch_dev, bytes([0x5A]) * (4 * n))
        tc, cptr, csl = _device_bytes(torch_dev, bytes([0x5A]) * (4 * n))
        if cap == n:   # capacity == n passes
            assert ctx.value_census_device(vptr, n, uptr, cptr, cap) == (n, 0)
            assert np.array_equal(_read(tu, usl, np.float32), want[0])
            continue
        with pytest.raises(ife.IfeError) as e:
            ctx.value_census_device(vptr, n, uptr, cptr, cap)
        assert e.value.code == ife.E_ARG and str(n) in str(e.value) and str(n - 1) in str(e.value)
        assert (e.value.n_unique, e.value.n_nan) == (n, 0)
        assert (_read(tu, usl, np.uint8) == 0x5A).all() and (_read(tc, csl, np.uint8) == 0x5A).all()
        assert _guards_intact(tu, usl) and _guards_intact(tc, csl)
    # HOST: the same refusal leaves the arrays as they were
    lib = ife.load_library()
    import ctypes as C
    u, c = np.full(n, 9, np.float32), np.full(n, 9, np.uint32)
    nu, nn = C.c_int64(-1), C.c_int64(-1)
    rc = lib.ife_value_census_f32(ctx._h, values.ctypes.data, n, u.ctypes.data, c.ctypes.data, n - 1, C.byref(nu),
                                  C.byref(nn), ife.MEM_HOST)
    assert rc == ife.E_ARG and (nu.value, nn.value) == (n, 0) and (u == 9).all() and (c == 9).all()


@pytest.mark.parametrize("n", [SEG - 1, SEG, SEG + 1, 2 * SEG + 1])
def test_census_at_the_segment_size(ctx, torch_dev, n):
    rng = np.random.default_rng(n)
    _check_census(ctx, torch_dev, np.arange(n, dtype=np.float32))                     # every element a head
    _check_census(ctx, torch_dev, rng.integers(0, 9, n).astype(np.float32))


def test_census_runs_across_segment_seams(ctx, torch_dev):
    """Sorted, the array is 200 x 1, 112 x 2 (over the seam at 256), 600 x 3 (over two seams) and
    one 4 that is the last element."""
    values = np.concatenate([np.full(200, 1), np.full(112, 2), np.full(600, 3), [4]]).astype(np.float32)
    want = _check_census(ctx, torch_dev, np.random.default_rng(5).permutation(values))
    assert list(want[1]) == [200, 112, 600, 1]
    # a head that is the first element of a segment, and one that is its last
    values = np.concatenate([np.full(SEG, 1), np.full(SEG - 1, 2), [3], np.full(5, 4)]).astype(np.float32)
    assert list(_check_census(ctx, torch_dev, values)[1]) == [SEG, SEG - 1, 1, 5]


def test_census_more_segments_than_a_scan_chunk(ctx):
    """4097 segments and a partial one: more than the 4096 waves of the two segment walks, so waves
    0 and 1 take a second segment.  Five values in long runs over thousands of segments, 3000
    distinct values in the middle of the sorted array, and 3000 more at its end, whose heads lie on
    both sides of the seam between the two chunks of the scan (sorted position 4096 * 256)."""
    n = SCAN_CHUNK * SEG + SEG + 7
    rng = np.random.default_rng(43)
    values = rng.integers(0, 5, n).astype(np.float32)
    values[:3000] = np.float32(2.5) + np.arange(3000, dtype=np.float32) / np.float32(8192)   # inside (2, 3)
    values[3000:6000] = np.float32(9) + np.arange(3000, dtype=np.float32)
    want = V.value_census(values)
    assert want[0].size == 6005 and n - 3000 < SCAN_CHUNK * SEG < n
    _census_equal(ctx.value_census(values), want)


def test_census_more_runs_than_the_runs_grid(ctx):
    """census_runs_kernel walks 1024 workgroups of 256 lanes, 262 144 runs a trip: 300 000 distinct
    values, some of them twice, so that lanes take a second run."""
    rng = np.random.default_rng(46)
    values = np.concatenate([np.arange(300000), rng.integers(0, 300000, 5000)]).astype(np.float32) - np.float32(1000)
    values = rng.permutation(values)
    want = V.value_census(values)
    assert want[0].size == 300000 and want[1].max() >= 2
    _census_equal(ctx.value_census(values), want)


def test_census_zeros_nans_infinities_and_denormals(ctx, torch_dev):
    d1, d2 = np.uint32(1).view(np.float32), np.uint32(2).view(np.float32)
    values = np.array([0.0, -0.0, NAN_POS, d2, -0.0, NAN_NEG, d1, np.inf, -np.inf, NAN_POS, d1, -d1, 7.0, 7.0],
                      np.float32)
    want = _check_census(ctx, torch_dev, values)
    assert want[2] == 3
    assert list(want[0].view(np.uint32)) == [0xff800000, 0x80000001, 0, 1, 2, 0x40e00000, 0x7f800000]
    assert list(want[1]) == [1, 1, 3, 2, 1, 2, 1]
    # the last run ends where the positive NaNs begin; NaNs of one sign only, and NaNs alone
    rng = np.random.default_rng(44)
    big = rng.integers(-3, 4, 3 * SEG + 5).astype(np.float32)
    big[rng.random(big.size) < 0.2] = NAN_POS
    big[rng.random(big.size) < 0.2] = NAN_NEG
    big[rng.random(big.size) < 0.1] = np.float32(-0.0)
    want = _check_census(ctx, torch_dev, big)
    bits = big.view(np.uint32)
    assert (bits == 0x7fc00001).sum() > 64 and (bits == 0xffc00000).sum() > 64     # more than a wave of either sign
    assert int(want[1].sum()) + want[2] == big.size
    _check_census(ctx, torch_dev, np.where(np.arange(300) % 3 == 0, NAN_POS, np.float32(1)).astype(np.float32))
    _check_census(ctx, torch_dev, np.where(np.arange(300) % 3 == 0, NAN_NEG, np.float32(1)).astype(np.float32))
    u, c, nn = ctx.value_census(np.array([NAN_NEG, NAN_POS, NAN_POS], np.float32))
    assert u.size == 0 and c.size == 0 and nn == 3
    u, c, nn = ctx.value_census(np.array([-0.0, 0.0, -0.0], np.float32))
    assert list(u.view(np.uint32)) == [0] and list(c) == [3] and nn == 0


def test_census_refusals(ife, ctx, torch_dev):
    values = np.arange(8, dtype=np.float32)
    tv, vptr, _ = _device_bytes(torch_dev, values.tobytes())
    to, optr, osl = _device_bytes(torch_dev, bytes(64))
    for args in ((vptr + 2, 7), (vptr, 8, optr + 2, optr + 32, 4), (vptr, 8, optr, optr + 34, 4),   # misaligned
                 (vptr, 8, optr, None, 4), (vptr, 8, None, None, 4), (None, 8)):                    # null pointers
        with pytest.raises(ife.IfeError) as e:
            ctx.value_census_device(*args)
        assert e.value.code == ife.E_ARG
    with pytest.raises(ife.IfeError) as e:
        ife.Context._census(ctx, vptr, 2 ** 32, None, None, 0, ife.MEM_DEVICE)
    assert e.value.code == ife.E_SIZE


# ---- threshold ----------------------------------------------------------------------------------------
def _check_threshold(ctx, torch_dev, image, low, high, offsets=((0, 0),)):
    image = np.ascontiguousarray(image, np.float32)
    want, count = V.threshold_mask(image, low, high)
    mask, got = ctx.threshold_mask(image, low, high)
    assert mask.dtype == np.uint8 and mask.shape == image.shape and np.array_equal(mask, want) and got == count
    for ioff, moff in offsets:
        ti, iptr, _ = _device_bytes(torch_dev, image.tobytes(), offset=ioff)
        tm, mptr, msl = _device_bytes(torch_dev, bytes([0x5A]) * image.size, offset=moff)
        assert ctx.threshold_mask_device(iptr, image.size, low, high, mptr) == count
        assert np.array_equal(_read(tm, msl, np.uint8), want.reshape(-1)) and _guards_intact(tm, msl)
    return want


def test_threshold_bounds_zeros_and_nans(ctx, torch_dev):
    d = np.uint32(5).view(np.float32)
    nxt = np.nextafter(np.float32(2), np.float32(3))
    prv = np.nextafter(np.float32(1), np.float32(0))
    img = np.array([1.0, 2.0, nxt, prv, -0.0, 0.0, d, -d, NAN_POS, NAN_NEG, np.inf, -np.inf, 1.5, -1.5], np.float32)
    assert list(_check_threshold(ctx, torch_dev, img, 1.0, 2.0)) == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    assert list(_check_threshold(ctx, torch_dev, img, 1.5, 1.5)) == [0] * 12 + [1, 0]                # low == high
    assert list(_check_threshold(ctx, torch_dev, img, -np.inf, np.inf)) == [1] * 8 + [0, 0] + [1] * 4
    assert list(_check_threshold(ctx, torch_dev, img, 0.0, 1.0)) == [1, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert list(_check_threshold(ctx, torch_dev, img, -0.0, -0.0)) == [0, 0, 0, 0, 1, 1] + [0] * 8
    assert list(_check_threshold(ctx, torch_dev, img, d, 1.0)) == [1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert list(_check_threshold(ctx, torch_dev, img, -d, d)) == [0, 0, 0, 0, 1, 1, 1, 1] + [0] * 6
    assert list(_check_threshold(ctx, torch_dev, img, np.inf, np.inf)) == [0] * 10 + [1, 0, 0, 0]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 259, 1031])
def test_threshold_lengths_and_alignments(ctx, torch_dev, n):
    """Every length class of the 16-byte pieces, from image sub-ranges that start 0 .. 3 elements
    beyond a 16-byte boundary onto masks at every byte offset."""
    rng = np.random.default_rng(n)
    img = rng.normal(0, 2, n).astype(np.float32)
    img[rng.random(n) < 0.1] = NAN_POS
    offsets = [(4 * a, b) for a in range(4) for b in range(4)]
    want = _check_threshold(ctx, torch_dev, img, -1.0, 1.5, offsets)
    assert n < 8 or 0 < want.sum() < n


def test_threshold_beyond_its_grid(ctx, torch_dev):
    """2048 workgroups of 256 lanes take 2 097 152 elements in pieces of four in one trip: 1203 more,
    from an image that starts one element beyond a 16-byte boundary."""
    n = 2048 * 256 * 4 + 1203
    rng = np.random.default_rng(45)
    img = rng.integers(-5, 6, n).astype(np.float32)
    want = _check_threshold(ctx, torch_dev, img, -1.0, 2.0, [(4, 3)])
    assert want[-1203:].sum() > 300 and want[:1203].sum() > 300


def test_threshold_refusals(ife, ctx, torch_dev):
    img = np.arange(16, dtype=np.float32)
    ti, iptr, _ = _device_bytes(torch_dev, img.tobytes())
    tm, mptr, msl = _device_bytes(torch_dev, bytes([0x5A]) * 16)
    lib = ife.load_library()
    import ctypes as C
    for low, high in ((2.0, 1.0), (float("nan"), 1.0), (1.0, float("nan")), (3e-45, 1e-45)):
        rc = lib.ife_threshold_mask(ctx._h, iptr, 16, low, high, mptr, None, ife.MEM_DEVICE)
        assert rc == ife.E_ARG, (low, high)
    assert lib.ife_threshold_mask(ctx._h, iptr, 0, 0.0, 1.0, mptr, None, ife.MEM_DEVICE) == ife.E_SIZE
    assert lib.ife_threshold_mask(ctx._h, iptr, 2 ** 40 + 1, 0.0, 1.0, mptr, None, ife.MEM_DEVICE) == ife.E_SIZE
    assert lib.ife_threshold_mask(ctx._h, None, 16, 0.0, 1.0, mptr, None, ife.MEM_DEVICE) == ife.E_ARG
    assert lib.ife_threshold_mask(ctx._h, iptr, 16, 0.0, 1.0, None, None, ife.MEM_DEVICE) == ife.E_ARG
    assert lib.ife_threshold_mask(ctx._h, iptr, 16, 0.0, 1.0, iptr + 60, None, ife.MEM_DEVICE) == ife.E_ARG  # overlap
    assert lib.ife_threshold_mask(ctx._h, iptr, 16, 0.0, 1.0, iptr - 15, None, ife.MEM_DEVICE) == ife.E_ARG
    assert (_read(tm, msl, np.uint8) == 0x5A).all()
    assert np.array_equal(_read(ti, slice(GUARD, GUARD + 64), np.float32), img)
    # a NULL count is legal
    assert lib.ife_threshold_mask(ctx._h, iptr, 16, 3.0, 5.0, mptr, None, ife.MEM_DEVICE) == 0
    assert list(_read(tm, msl, np.uint8)) == [0, 0, 0, 1, 1, 1] + [0] * 10
    del C


# ---- coverage -----------------------------------------------------------------------------------------
def _device_coverage(ife, ctx, torch_dev, mask, rois, ends):
    rois = np.asarray(rois, np.int64).reshape(-1, 6)
    tm, mptr, _ = _device_bytes(torch_dev, mask.tobytes())
    tr, rptr, _ = _device_bytes(torch_dev, rois.tobytes() if rois.size else bytes(48))
    code = ife.U8 if mask.dtype == np.uint8 else ife.U16
    return ctx.roi_coverage_device(mptr, code, mask.shape, rptr if rois.size else None, rois.shape[0], ends)


def _both(ife, ctx, torch_dev, mask, rois, ends):
    want = V.roi_coverage(mask, rois, ends)
    for got in (ctx.roi_coverage(mask, np.asarray(rois, np.int64).reshape(-1, 6), ends),
                _device_coverage(ife, ctx, torch_dev, mask, rois, ends)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (got, want)
    assert (np.diff(want[0]) >= 0).all() and (want[1] <= np.minimum(want[0], want[2])).all()
    return want


@pytest.fixture(scope="module")
def mask37():
    return (np.random.default_rng(51).random(SHAPE) < 0.45).astype(np.uint8)


def test_coverage_box_rows_and_words(ife, ctx, torch_dev, mask37):
    nz, ny, nx = SHAPE
    rows = [
        [3, 0, 0, 20, 1, 1],      # bits 3 .. 22: inside one word
        [0, 0, 0, 32, 1, 1],      # bit 0 to bit 31 of word 0
        [0, 0, 0, 1, 1, 1],       # starts at bit 0
        [31, 0, 0, 1, 1, 1],      # ends at bit 31
        [30, 0, 0, 4, 1, 1],      # two words
        [0, 1, 0, 37, 1, 1],      # row 1 is bits 37 .. 73: two words, none of them whole
        [0, 1, 1, 37, 1, 1],      # row 6 is bits 222 .. 258: three words
        [0, 2, 1, 37, 3, 2],      # rows that straddle words, rows and a plane
        [36, 4, 2, 1, 1, 1],      # the last voxel: the tail word
    ]
    for k in range(len(rows)):    # each alone, then all of them
        want = _both(ife, ctx, torch_dev, mask37, rows[k:k + 1], [1])
        assert want[0][0] == np.prod(rows[k][3:])
    _both(ife, ctx, torch_dev, mask37, rows, list(range(len(rows) + 1)))


def test_coverage_whole_volume_unit_boxes_duplicates_and_sizes(ife, ctx, torch_dev, mask37):
    nz, ny, nx = SHAPE
    want = _both(ife, ctx, torch_dev, mask37, [[0, 0, 0, nx, ny, nz]], [1])
    assert want[0][0] == mask37.size and want[1][0] == want[2] == int(mask37.sum())
    rng = np.random.default_rng(52)
    units = [[int(rng.integers(0, nx)), int(rng.integers(0, ny)), int(rng.integers(0, nz)), 1, 1, 1] for _ in range(40)]
    units += units[:7]                                                     # duplicates
    _both(ife, ctx, torch_dev, mask37, units, [0, 5, 5, 40, 47])           # a 0, a repeat and n_rois
    mixed = [[0, 0, 0, 5, 2, 1], [2, 1, 0, 33, 3, 2], [2, 1, 0, 33, 3, 2], [30, 0, 1, 7, 5, 2], [4, 4, 2, 20, 1, 1]]
    want = _both(ife, ctx, torch_dev, mask37, mixed, [1, 2, 3, 3, 5])
    assert want[0][1] == want[0][2] == want[0][3]                          # the duplicate adds nothing
    _both(ife, ctx, torch_dev, mask37, mixed, [5])
    _both(ife, ctx, torch_dev, mask37, mixed, [0])
    _both(ife, ctx, torch_dev, mask37, mixed, [0] * 64)


def test_coverage_no_boxes_empty_masks_and_uint16(ife, ctx, torch_dev, mask37):
    want = _both(ife, ctx, torch_dev, mask37, np.empty((0, 6), np.int64), [0, 0])
    assert list(want[0]) == [0, 0] and want[2] == int(mask37.sum())
    empty = np.zeros(SHAPE, np.uint8)
    want = _both(ife, ctx, torch_dev, empty, [[1, 1, 1, 9, 2, 2]], [1])
    assert (want[0][0], want[1][0], want[2]) == (36, 0, 0)
    m16 = np.where(mask37 != 0, 256, 0).astype(np.uint16)                  # the low byte alone is 0
    want = _both(ife, ctx, torch_dev, m16, [[1, 1, 1, 9, 2, 2], [0, 0, 0, 37, 1, 1]], [1, 2])
    assert want[2] == int(mask37.sum()) and want[1][1] > 0


def test_coverage_of_33_voxels(ife, ctx, torch_dev):
    """Two words, the second with one voxel; as a row, a column and a pillar."""
    for shape in ((1, 1, 33), (1, 33, 1), (33, 1, 1), (3, 11, 1)):
        mask = (np.arange(33).reshape(shape) % 3 != 0).astype(np.uint8)
        nz, ny, nx = shape
        _both(ife, ctx, torch_dev, mask, [[nx - 1, ny - 1, nz - 1, 1, 1, 1], [0, 0, 0, nx, ny, nz]], [1, 2])
        _both(ife, ctx, torch_dev, mask, [[0, 0, 0, 1, 1, 1]], [1])


def test_coverage_refuses_boxes_outside(ife, ctx, torch_dev, mask37):
    import ctypes as C
    nz, ny, nx = SHAPE
    good = [1, 1, 1, 5, 2, 2]
    lib = ife.load_library()
    d = ife._desc(SHAPE, (1.0, 1.0, 1.0))
    tm, mptr, _ = _device_bytes(torch_dev, mask37.tobytes())
    for bad in ([nx - 4, 1, 1, 5, 2, 2], [1, ny - 1, 1, 5, 2, 2], [1, 1, nz - 1, 5, 2, 2],   # one voxel outside
                [-1, 1, 1, 5, 2, 2], [1, 1, 1, 0, 2, 2], [1, 1, 1, 5, 2, -1]):
        rois = np.array([good, good, bad, good], np.int64)
        tr, rptr, _ = _device_bytes(torch_dev, rois.tobytes())
        for mem, mp, rp in ((ife.MEM_HOST, mask37.ctypes.data, rois.ctypes.data), (ife.MEM_DEVICE, mptr, rptr)):
            ends = (C.c_int64 * 2)(1, 2)     # the bad box lies beyond every round: refused all the same
            vis, hit, reg = (C.c_int64 * 2)(-7, -7), (C.c_int64 * 2)(-7, -7), C.c_int64(-7)
            rc = lib.ife_roi_coverage(ctx._h, mp, ife.U8, C.byref(d), rp, 4, ends, 2, vis, hit, C.byref(reg), mem)
            assert rc == ife.E_ARG, (bad, mem)
            assert list(vis) == [-7, -7] and list(hit) == [-7, -7] and reg.value == -7
    # the library's own refusals of the rounds, a misaligned pointer and a null one
    rois = np.array([good], np.int64)
    tr, rptr, _ = _device_bytes(torch_dev, rois.tobytes())
    vis, hit = (C.c_int64 * 65)(), (C.c_int64 * 65)()
    call = lambda mp, rp, n, ends, mem: lib.ife_roi_coverage(  # noqa: E731
        ctx._h, mp, ife.U8, C.byref(d), rp, n, (C.c_int64 * len(ends))(*ends) if ends else None, len(ends), vis, hit,
        None, mem)
    assert call(mptr, rptr, 1, [1], ife.MEM_DEVICE) == 0 and vis[0] == 20          # a NULL region_size is legal
    assert call(mptr, rptr, 1, [1, 0], ife.MEM_DEVICE) == ife.E_ARG
    assert call(mptr, rptr, 1, [2], ife.MEM_DEVICE) == ife.E_ARG
    assert call(mptr, rptr, 1, [], ife.MEM_DEVICE) == ife.E_ARG
    assert call(mptr, rptr, 1, [0] * 65, ife.MEM_DEVICE) == ife.E_ARG
    assert call(mptr, rptr + 4, 1, [1], ife.MEM_DEVICE) == ife.E_ARG
    assert call(mptr, None, 1, [1], ife.MEM_DEVICE) == ife.E_ARG
    assert call(None, rptr, 1, [1], ife.MEM_DEVICE) == ife.E_ARG
    m16 = mask37.astype(np.uint16)
    t16, p16, _ = _device_bytes(torch_dev, m16.tobytes(), offset=1)
    assert lib.ife_roi_coverage(ctx._h, p16, ife.U16, C.byref(d), rptr, 1, (C.c_int64 * 1)(1), 1, vis, hit, None,
                                ife.MEM_DEVICE) == ife.E_ARG


def test_coverage_beyond_the_painter_grid(ife, ctx, torch_dev):
    """4500 boxes of 1 x 8 x 8: the painter's grid holds 4096 waves of one box each, so waves take
    a second box; (20, 24, 70) has 33600 voxels, 132 groups of the plane kernel."""
    shape = (20, 24, 70)
    rng = np.random.default_rng(53)
    mask = (rng.random(shape) < 0.3).astype(np.uint8)
    n = 4500
    rois = np.stack([rng.integers(0, 70, n), rng.integers(0, 17, n), rng.integers(0, 13, n),
                     np.ones(n, np.int64), np.full(n, 8), np.full(n, 8)], 1).astype(np.int64)
    want = _both(ife, ctx, torch_dev, mask, rois, [100, 4200, n])
    assert want[0][1] < want[0][2] < mask.size        # the boxes beyond the first trip add voxels


def test_coverage_beyond_the_plane_and_count_grids(ife, ctx, torch_dev):
    """(130, 256, 256): 33 280 groups of 256 voxels for the 8192 waves of the plane kernel (a fifth
    trip, not all waves on it) and 266 240 words for the 262 144 lanes of the count kernel; boxes at
    both ends of the volume and in the words of the second trip."""
    shape = (130, 256, 256)
    rng = np.random.default_rng(55)
    mask = (rng.random(shape) < 0.25).astype(np.uint8)
    rois = [[0, 0, 0, 40, 3, 2], [200, 250, 128, 56, 6, 2], [100, 100, 60, 53, 53, 41], [255, 255, 129, 1, 1, 1]]
    want = _both(ife, ctx, torch_dev, mask, rois, [1, 2, 4])
    assert want[0][1] - want[0][0] == 56 * 6 * 2 and want[2] == int(mask.sum())


def test_coverage_more_boxes_than_the_box_check_grid(ife, ctx, torch_dev):
    """coverage_box_check_kernel walks 2048 workgroups of 256 lanes: 524 289 boxes of one voxel on the
    device, the last of them one voxel outside the volume: IFE_E_ARG; repaired, the counts are those of
    the distinct voxels."""
    shape = (16, 64, 70)
    rng = np.random.default_rng(56)
    mask = (rng.random(shape) < 0.5).astype(np.uint8)
    n = 2048 * 256 + 1
    lin = rng.integers(0, mask.size // 2, n)          # the upper half of the volume stays unvisited
    rois = np.ones((n, 6), np.int64)
    rois[:, 0], rois[:, 1], rois[:, 2] = lin % 70, lin // 70 % 64, lin // (70 * 64)
    good = rois[-1].copy()
    rois[-1, :3] = (70, 0, 0)
    tm, mptr, _ = _device_bytes(torch_dev, mask.tobytes())
    tr, rptr, _ = _device_bytes(torch_dev, rois.tobytes())
    with pytest.raises(ife.IfeError) as e:
        ctx.roi_coverage_device(mptr, ife.U8, shape, rptr, n, [10, n])
    assert e.value.code == ife.E_ARG
    rois[-1] = good
    tr, rptr, _ = _device_bytes(torch_dev, rois.tobytes())
    visited, hits, region = ctx.roi_coverage_device(mptr, ife.U8, shape, rptr, n, [10, n])
    seen = np.unique(lin)
    assert visited[1] == seen.size and hits[1] == int(mask.reshape(-1)[seen].sum()) and region == int(mask.sum())
    assert visited[0] == np.unique(lin[:10]).size and hits[0] == int(mask.reshape(-1)[np.unique(lin[:10])].sum())


# ---- end to end ---------------------------------------------------------------------------------------
def test_threshold_draws_and_coverage_end_to_end(ctx, synth):
    shape = (21, 33, 40)
    rng = np.random.default_rng(54)
    image = rng.normal(0, 1, shape).astype(np.float32)
    low, high = np.float32(-0.43), np.float32(0.43)               # about a third of a standard normal
    mask, count = ctx.threshold_mask(image, low, high)
    want_mask, want_count = V.threshold_mask(image, low, high)
    assert np.array_equal(mask, want_mask) and count == want_count
    assert 0.28 < count / image.size < 0.39
    rois, n_adm = ctx.random_rois(mask, 2000, (7, 5, 3), seed=7)
    want_rois, want_adm = S.random_rois(want_mask, 2000, (7, 5, 3), seed=7)
    assert np.array_equal(rois, want_rois) and np.array_equal(n_adm, want_adm)
    got = ctx.roi_coverage(mask, rois[0], V.ROUND_ENDS)
    want = V.roi_coverage(want_mask, want_rois[0], V.ROUND_ENDS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] == count
    assert got[0][0] < got[0][-1] <= image.size and 0 < got[1][0] < got[1][-1] <= count
