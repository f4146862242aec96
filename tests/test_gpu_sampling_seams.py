"""The seams of the sampling kernels (csrc/sampling_kernels.hpp, launched from
csrc/sampling_capi.inc) that the shapes of tests/test_gpu_sampling.py do not reach: gathered rows
of more than 64 pieces and of a piece or less at every alignment, more rows and more boxes than a
capped grid holds, rows of exactly one or two segments and of one voxel, idle waves and the capped
grid of the count pass, the second trip of the select kernel, and all 32 value sets.

Everything is integer or bit copying: equality, no tolerance.  The checkers are
tests/sampling_oracle.py and numpy.  Every test names the constant it crosses and restates the
crossing with the literal number, so that a later change of a shape cannot drop the coverage
unnoticed.  A test on more than about a million voxels or boxes runs in a context of its own."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (6, 7, 70)
GUARD = 64
ELEM_DTYPES = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def _device_bytes(torch_dev, payload, offset=0, fill=0xA5):
    """A device byte buffer [guard | offset | payload | guard], all guard bytes `fill`; returns
    (tensor, pointer of the payload, slice of the payload)."""
    torch, dev = torch_dev
    raw = np.full(GUARD + offset + len(payload) + GUARD, fill, np.uint8)
    raw[GUARD + offset:GUARD + offset + len(payload)] = np.frombuffer(payload, np.uint8)
    t = torch.from_numpy(raw).to(dev)
    torch.cuda.synchronize()
    return t, t.data_ptr() + GUARD + offset, slice(GUARD + offset, GUARD + offset + len(payload))


def _volume(shape, es, seed):
    """Elements of `es` bytes whose bytes all differ from their neighbours' (any bit pattern is
    legal: bits are copied)."""
    raw = np.random.default_rng(seed).integers(1, 250, tuple(shape) + (es,), dtype=np.uint8)
    return np.ascontiguousarray(raw).view(ELEM_DTYPES[es]).reshape(shape)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _gather_to_device(ctx, torch_dev, src, s_ptr, boxes, offset):
    """extract_rois_device with dst `offset` bytes behind a 16-byte boundary: the payload and
    whether the guards are intact"""
    es = src.dtype.itemsize
    rois = np.array(boxes, np.int64).reshape(-1, 6)
    r_t, r_ptr, _ = _device_bytes(torch_dev, rois.tobytes())
    d_t, d_ptr, where = _device_bytes(torch_dev, bytes(int(rois.shape[0] * np.prod(rois[0, 3:])) * es), offset)
    assert d_ptr % 16 == offset
    ctx.extract_rois_device(s_ptr, es, src.shape, r_ptr, rois.shape[0], d_ptr)
    back = d_t.cpu().numpy()
    return back[where].tobytes(), bool((back[:where.start] == 0xA5).all() and (back[where.stop:] == 0xA5).all())


# ---- 5. gather: rows longer than one wave trip ---------------------------------------------------
# csrc/sampling_kernels.hpp sampling_gather_kernel: a wave takes a row of a box and its piece loop
# strides by the 64 lanes.
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_gather_rows_longer_than_a_wave_trip(ctx, torch_dev, es):
    epp = 16 // es
    sx = 65 * epp + 3
    shape = (3, 3, 66 * epp + 9)
    src = _volume(shape, es, 71)
    boxes = [[x0, y0, z0, sx, 2, 2] for x0 in range(6) for y0, z0 in ((0, 0), (1, 1))]
    assert all(b[0] + sx <= shape[2] for b in boxes)
    want = S.extract_rois(src, boxes)
    assert _same_bits(ctx.extract_rois(src, boxes), want)
    s_t, s_ptr, _ = _device_bytes(torch_dev, src.tobytes())
    nrows = len(boxes) * 4
    for offset in range(0, 16, es):
        # the kernel's arithmetic: rows whose head is at most 3 elements have 65 pieces or more
        nb = [(sx - min(sx, ((0 - (offset + r * sx * es)) & 15) // es)) // epp for r in range(nrows)]
        assert min(nb) >= 64 and max(nb) > 64
        if offset == 0:
            assert nb[0] > 64
        got, intact = _gather_to_device(ctx, torch_dev, src, s_ptr, boxes, offset)
        assert got == want.tobytes() and intact, offset


# ---- 6. gather: rows of a piece or less ----------------------------------------------------------
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_gather_short_rows_at_every_alignment(ctx, torch_dev, es):
    """csrc/sampling_kernels.hpp sampling_gather_kernel: head = min(sx, ...), nb whole pieces of EPP =
    16 / ES elements, a tail.  Widths 1, 15, 16, 17 and 33: rows shorter than their head would be,
    without a piece, of exactly one (one-byte elements), with a head and a tail only; dst at every
    element-aligned offset inside 16 bytes, so that a store behind the last row meets a guard."""
    assert 1 * es < 16 <= 16 * es and 15 * 1 < 16 < 17 * 1      # below, at and above a piece for ES = 1
    src = _volume(SHAPE, es, 72)
    s_t, s_ptr, _ = _device_bytes(torch_dev, src.tobytes())
    nz, ny, nx = SHAPE
    for w in (1, 15, 16, 17, 33):
        boxes = [[x0, y0, z0, w, 2, 2] for x0, y0, z0 in ((0, 0, 0), (1, 2, 1), (3, 5, 4), (nx - w, ny - 2, nz - 2),
                                                           (nx - w - 1, 0, 3), (1, 2, 1))]
        want = S.extract_rois(src, boxes)
        assert _same_bits(ctx.extract_rois(src, boxes), want), w
        for offset in range(0, 16, es):
            got, intact = _gather_to_device(ctx, torch_dev, src, s_ptr, boxes, offset)
            assert got == want.tobytes() and intact, (w, offset)


# ---- 7. gather: more rows than the grid ----------------------------------------------------------
def test_gather_more_rows_than_the_grid_cap(ctx):
    """csrc/sampling_kernels.hpp SAMPLING_GATHER_GRID_CAP = 4096 workgroups of REGION_WAVES = 4
    waves, a row each: 700 boxes of 5 x 5 x 5 are 17 500 rows, more than the 16 384 of a trip."""
    n_boxes = 700
    assert n_boxes * 5 * 5 == 17500 > 4 * 4096
    rng = np.random.default_rng(73)
    nz, ny, nx = SHAPE
    src = _volume(SHAPE, 2, 74)
    boxes = np.stack([rng.integers(0, nx - 4, n_boxes), rng.integers(0, ny - 4, n_boxes), rng.integers(0, nz - 4, n_boxes)]
                     + [np.full(n_boxes, 5)] * 3, axis=1).astype(np.int64)
    boxes[-3:] = boxes[0]                                    # repeated; 700 boxes in 66 * 3 * 2 places overlap
    assert len({tuple(b) for b in boxes}) < n_boxes
    assert _same_bits(ctx.extract_rois(src, boxes), S.extract_rois(src, boxes))


# ---- 8. box check: more boxes than its grid ------------------------------------------------------
def test_box_check_more_boxes_than_its_grid(ife, torch_dev):
    """csrc/sampling_capi.inc ife_extract_rois: sampling_box_check_kernel runs at most 2048
    workgroups of 256 lanes, a box each.  The box that leaves the volume is the last one, which only
    a second trip sees; nothing may be written before every box is checked."""
    torch, _ = torch_dev
    n = 2048 * 256 + 12
    assert n == 524300 > 2048 * 256
    nz, ny, nx = SHAPE
    rng = np.random.default_rng(75)
    src = _volume(SHAPE, 2, 76)
    x, y, z = rng.integers(0, nx, n), rng.integers(0, ny, n), rng.integers(0, nz, n)
    rois = np.stack([x, y, z, np.ones(n, np.int64), np.ones(n, np.int64), np.ones(n, np.int64)], axis=1).astype(np.int64)
    want = src[z, y, x]
    rois[-1, 0] = nx                                         # one voxel beyond the row
    s_t, s_ptr, _ = _device_bytes(torch_dev, src.tobytes())
    r_t, r_ptr, r_where = _device_bytes(torch_dev, rois.tobytes())
    d_t, d_ptr, where = _device_bytes(torch_dev, bytes([0x3C]) * (2 * n))
    with ife.Context(0) as c:
        with pytest.raises(ife.IfeError) as e:
            c.extract_rois_device(s_ptr, 2, SHAPE, r_ptr, n, d_ptr)
        assert e.value.code == ife.E_ARG
        back = d_t.cpu().numpy()
        assert (back[where] == 0x3C).all() and (back[:where.start] == 0xA5).all() and (back[where.stop:] == 0xA5).all()
        # the box repaired in place
        last_x = r_where.start + 48 * (n - 1)
        r_t[last_x:last_x + 8] = torch.from_numpy(np.frombuffer(np.int64(x[-1]).tobytes(), np.uint8).copy()).to(r_t.device)
        torch.cuda.synchronize()
        c.extract_rois_device(s_ptr, 2, SHAPE, r_ptr, n, d_ptr)
        back = d_t.cpu().numpy()
    got = back[where].view(src.dtype)
    assert np.array_equal(got[:2048 * 256], want[:2048 * 256]), "the first trip of the gather's rows"
    assert np.array_equal(got[2048 * 256:], want[2048 * 256:]), "the boxes behind 2048 * 256"
    assert (back[:where.start] == 0xA5).all() and (back[where.stop:] == 0xA5).all()


# ---- 9. count and select: row shapes ------------------------------------------------------------
def _check(ctx, mask, n_draws, size, **kw):
    """Both calls against the oracle; returns the oracle's positions."""
    want, counts = S.sample_positions(mask, n_draws, size, **kw)
    pos, n = ctx.sample_positions(mask, n_draws, size, **kw)
    assert np.array_equal(n, counts)
    assert pos.shape == want.shape and np.array_equal(pos, want)
    rois, n = ctx.random_rois(mask, n_draws, size, **kw)
    assert np.array_equal(n, counts)
    assert np.array_equal(rois, S.boxes_of(want, mask.shape, size))
    return want


def _labels(shape, dtype, seed):
    """Labels 0 .. 4 in equal numbers in a random order (uint16: 300 for some of the 2, whose low
    byte alone would be 44)."""
    n = int(np.prod(shape))
    m = np.random.default_rng(seed).permutation(n) % 5
    if dtype == np.uint16:
        m = np.where((m == 2) & (np.arange(n) % 2 == 0), 300, m)
    return m.astype(dtype).reshape(shape)


def _count_grid(nseg):
    """(blocks, waves, per) of sampling_count_kernel: csrc/sampling_capi.inc sampling_draw launches
    min(max(ceil(nseg / (4 * SAMPLING_COUNT_RUN)), 1), 1 << 18) workgroups of 4 waves, and a wave
    takes per = ceil(nseg / waves) consecutive segments."""
    blocks = min(max((nseg + 4 * 8 - 1) // (4 * 8), 1), 1 << 18)
    return blocks, 4 * blocks, (nseg + 4 * blocks - 1) // (4 * blocks)


ROW_SHAPES = [(5, 6, 64), (5, 6, 128), (5, 6, 1), (5, 6, 37), (1, 9, 70), (9, 1, 70), (1, 1, 33), (3, 11, 1)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_count_and_select_row_shapes(ctx, shape, dtype):
    """Rows of exactly one and two segments of 64 voxels, of less than one, of one voxel; ny = 1
    and nz = 1, where the count pass's carried (bx, y, z) wraps at every step; and so few segments
    that waves of the count pass have none (s0 >= s1)."""
    nz, ny, nx = shape
    nseg = (nx + 63) // 64 * ny * nz
    blocks, waves, per = _count_grid(nseg)
    if shape == (1, 1, 33):
        assert nseg == 1 and (blocks, per) == (1, 1)        # waves 1 .. 3 have no segment
    if shape == (3, 11, 1):
        assert nseg == 33 and blocks == 2 and per == 5
        assert 7 * per >= nseg > 6 * per                    # wave 7 has no segment, wave 6 three
    if shape == (5, 6, 64):
        assert nx == 64 and nseg == 30 and (blocks, per) == (1, 8)   # whole segments; the last wave has six
    if shape == (5, 6, 128):
        assert nx == 128 and nseg == 60 and per == 8        # the SAMPLING_COUNT_RUN = 8 of an uncapped grid
    mask = _labels(shape, dtype, 81)
    mixed = (min(4, nx), min(3, ny), min(2, nz))            # even and odd extents where they fit
    for size in ((1, 1, 1), mixed):
        _check(ctx, mask, 130, size, seed=41)                                          # mask != 0
        _check(ctx, mask, 130, size, values=(3, 1), seed=42, stream=9)                 # the union
        _check(ctx, mask, 130, size, values=(3, 1, 3, 4), per_value=True, seed=43, stream=2)
        if dtype == np.uint16:
            _check(ctx, mask, 130, size, values=(300, 44, 2), per_value=False, seed=44)
            assert ctx.sample_positions(mask, 0, size, values=(44,))[1][0] == 0


# ---- 10. count: the capped grid -------------------------------------------------------------------
def test_count_capped_grid(ife):
    """csrc/sampling_capi.inc sampling_draw: the count pass has at most 1 << 18 workgroups of 4
    waves, SAMPLING_COUNT_RUN = 8 segments to a wave; beyond 8 * 4 * 2^18 = 8 388 608 segments the
    runs grow.  Rows of two voxels make a segment of every row: 8 405 000 segments, per = 9, and
    2053 chunks for scan_chunks_kernel (csrc/stats_kernels.hpp: SCAN_CHUNK = 4096, 256 threads,
    so 9 chunks to a thread)."""
    shape = (2050, 4100, 2)
    nz, ny, nx = shape
    nseg = (nx + 63) // 64 * ny * nz
    assert nseg == 8405000 > 8 * 4 * 2 ** 18 == 8388608
    blocks, waves, per = _count_grid(nseg)
    assert blocks == 1 << 18 and per == 9 > 8
    assert (nseg + 4095) // 4096 == 2053 > 256
    rng = np.random.default_rng(82)
    mask = (rng.random(shape) < 0.02).astype(np.uint8)      # value 1, sparse
    rows = mask.reshape(nseg, nx)
    rows[-20000:] = 1                                       # dense behind the uncapped grid's reach
    rows[-20000::7, 1] = 2                                  # value 2: there and in the first 64 rows only
    rows[:64] = 2
    with ife.Context(0) as c:
        for size in ((1, 1, 1), (2, 3, 3)):
            pos = _check(c, mask, 1000, size, seed=51)
            assert (pos // nx >= 8388608).any()
        # (2, 3, 3) admits no voxel of the plane z = 0; the first segments are seen by (1, 1, 1)
        pos = _check(c, mask, 1000, (1, 1, 1), values=(1, 2), per_value=True, seed=52, stream=3)
        assert (pos[1] // nx < 64).any() and (pos[1] // nx >= 8388608).any()
        assert (pos[0] // nx >= 8388608).any() and (pos[0] // nx < 8388608).any()
        assert (mask.reshape(-1)[pos[1]] == 2).all() and (mask.reshape(-1)[pos[0]] == 1).all()


# ---- 11. select: the second trip ------------------------------------------------------------------
def test_select_second_trip(ctx):
    """csrc/sampling_kernels.hpp SAMPLING_SELECT_GRID_CAP = 65536 workgroups of 4 waves, a draw
    each: 2 sets of 140 000 draws are 280 000 waves, 17 856 more than the 262 144 of a trip."""
    n_draws = 140000
    assert 2 * n_draws == 280000 > 4 * 65536 == 262144 and 2 * n_draws - 4 * 65536 == 17856
    mask = _labels(SHAPE, np.uint8, 83)
    kw = dict(values=(1, 2), per_value=True, seed=61, stream=5)
    want, counts = S.sample_positions(mask, n_draws, (5, 4, 3), **kw)
    pos, n = ctx.sample_positions(mask, n_draws, (5, 4, 3), **kw)
    assert np.array_equal(n, counts)
    assert np.array_equal(pos[0], want[0]), "set 0: first trip"
    assert np.array_equal(pos[1, :-17856], want[1, :-17856]), "set 1: first trip"
    assert np.array_equal(pos[1, -17856:], want[1, -17856:]), "set 1: the 17 856 draws of the second trip"
    rois, n = ctx.random_rois(mask, n_draws, (5, 4, 3), **kw)
    boxes = S.boxes_of(want, SHAPE, (5, 4, 3))
    assert np.array_equal(n, counts)
    assert np.array_equal(rois[0], boxes[0]), "set 0: first trip"
    assert np.array_equal(rois[1, :-17856], boxes[1, :-17856]), "set 1: first trip"
    assert np.array_equal(rois[1, -17856:], boxes[1, -17856:]), "set 1: the 17 856 boxes of the second trip"


# ---- 12. thirty-two sets --------------------------------------------------------------------------
def test_thirty_two_sets(ctx):
    """csrc/sampling_plan.hpp SAMPLING_MAX_VALUES = 32: set j's counts, bases and total stand at
    j * set_stride; the tests of tests/test_gpu_sampling.py have at most four sets."""
    rng = np.random.default_rng(84)
    values = [0, 255, 256, 300, 65535] + [int(v) for v in rng.choice(np.arange(1, 65535), 40, replace=False)
                                         if v not in (255, 256, 300)][:27]
    assert len(values) == len(set(values)) == 32
    n = int(np.prod(SHAPE))
    mask = np.array(values, np.uint16)[rng.permutation(n) % 32].reshape(SHAPE)
    flat = mask.reshape(-1)
    for size in ((1, 1, 1), (5, 4, 3)):
        pos = _check(ctx, mask, 65, size, values=values, per_value=True, seed=71, stream=11)
        assert pos.shape == (32, 65)
        for j, v in enumerate(values):
            assert (flat[pos[j]] == v).all(), (j, v)
        union = _check(ctx, mask, 65, size, values=values, seed=71, stream=11)
        assert union.shape == (1, 65)
        # the same value twice, in the first and in the last place: the same voxels, another stream
        twice = values[:31] + [values[0]]
        pos = _check(ctx, mask, 65, size, values=twice, per_value=True, seed=71, stream=11)
        assert (flat[pos[31]] == values[0]).all() and not np.array_equal(pos[0], pos[31])
