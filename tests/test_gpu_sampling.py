"""The sampling calls on the device (ife_sample_positions, ife_random_rois, ife_extract_rois)
against tests/sampling_oracle.py.  Nothing here has a tolerance: counts, positions, boxes and
copied bits are compared for equality.  The shapes are the smallest that reach every path: a row of
70 voxels crosses the 64-lane seam and ends in a partial segment; (44, 48, 70) has 4224 row
segments, more than one SCAN_CHUNK of 4096."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (6, 7, 70)
BIG = (44, 48, 70)
N_DRAWS = 257
GUARD = 64
DTYPES = (np.uint8, np.uint16)


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


def _guards_intact(t, sl, fill=0xA5):
    h = t.cpu().numpy()
    return (h[:sl.start] == fill).all() and (h[sl.stop:] == fill).all()


@pytest.fixture(scope="module")
def masks():
    """Label volumes 0 .. 4 (uint16: 200 and 300 too) of SHAPE, one per dtype."""
    rng = np.random.default_rng(21)
    m8 = rng.integers(0, 5, SHAPE).astype(np.uint8)
    m16 = m8.astype(np.uint16)
    m16[rng.random(SHAPE) < 0.1] = 200
    m16[rng.random(SHAPE) < 0.1] = 300   # the low byte alone would be 44
    return {np.uint8: m8, np.uint16: m16}


def _check(ctx, mask, n_draws, size, **kw):
    """Both calls against the oracle; returns the positions."""
    want, counts = S.sample_positions(mask, n_draws, size, **kw)
    pos, n = ctx.sample_positions(mask, n_draws, size, **kw)
    assert np.array_equal(n, counts)
    assert pos.shape == want.shape and np.array_equal(pos, want)
    rois, n = ctx.random_rois(mask, n_draws, size, **kw)
    assert np.array_equal(n, counts)
    assert np.array_equal(rois, S.boxes_of(want, mask.shape, size))
    return pos


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(1, 1, 1), (5, 4, 3)])
def test_value_modes(ctx, masks, dtype, size):
    mask = masks[dtype]
    _check(ctx, mask, N_DRAWS, size, seed=5)                                      # mask != 0
    _check(ctx, mask, N_DRAWS, size, values=(3, 1), seed=5, stream=9)             # the union
    pos = _check(ctx, mask, N_DRAWS, size, values=(3, 1, 3, 4), per_value=True, seed=5, stream=2)
    # sets 0 and 2 share their voxels but not their stream
    assert not np.array_equal(pos[0], pos[2])
    assert np.array_equal(pos[2], _check(ctx, mask, N_DRAWS, size, values=(3,), per_value=True, seed=5, stream=4)[0])
    if dtype == np.uint16:
        _check(ctx, mask, N_DRAWS, size, values=(3, 1, 3, 200), per_value=True, seed=5)
        _check(ctx, mask, N_DRAWS, size, values=(300, 44), seed=5)
        assert ctx.sample_positions(mask, 0, size, values=(44,))[1][0] == 0


def test_an_absent_value_is_refused_and_counted(ife, ctx, masks):
    """Value 200 does not occur in the uint8 data: IFE_E_ARG names set 3, the counts are written."""
    mask = masks[np.uint8]
    for fn in (ctx.sample_positions, ctx.random_rois):
        with pytest.raises(ife.IfeError) as e:
            fn(mask, N_DRAWS, (5, 4, 3), values=(3, 1, 3, 200), per_value=True, seed=5)
        assert e.value.code == ife.E_ARG and "set 3" in str(e.value) and "200" in str(e.value)
        want = [len(a) for a in S.admissible(mask, (5, 4, 3), (3, 1, 3, 200), True)]
        assert want[3] == 0 and min(want[:3]) > 0 and list(e.value.n_admissible) == want
    # without draws the same arguments are legal and give the counts alone
    pos, n = ctx.sample_positions(mask, 0, (5, 4, 3), values=(3, 1, 3, 200), per_value=True)
    assert pos.shape == (4, 0) and list(n) == want


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_possible_centre_and_none(ife, ctx, torch_dev, masks, dtype):
    nz, ny, nx = SHAPE
    mask = masks[dtype].copy()
    centre = (3 * ny + 3) * nx + 35
    mask.reshape(-1)[centre] = 2
    assert [len(a) for a in S.admissible(mask, (70, 7, 6))] == [1]
    pos = _check(ctx, mask, N_DRAWS, (70, 7, 6), seed=8)
    assert (pos == centre).all()
    mask.reshape(-1)[centre] = 0   # the only voxel that fits is background
    with pytest.raises(ife.IfeError) as e:
        ctx.random_rois(mask, 1, (70, 7, 6))
    assert e.value.code == ife.E_ARG and list(e.value.n_admissible) == [0]
    # a box longer than the row fits nowhere: counts written, the output untouched
    code = ife.U8 if dtype == np.uint8 else ife.U16
    tm, mptr, _ = _device_bytes(torch_dev, masks[dtype].tobytes())
    for fn, width in ((ctx.sample_positions_device, 1), (ctx.random_rois_device, 6)):
        to, optr, sl = _device_bytes(torch_dev, bytes([0x5A]) * (8 * width * N_DRAWS))
        with pytest.raises(ife.IfeError) as e:
            fn(mptr, code, SHAPE, optr, N_DRAWS, size=(71, 1, 1), seed=1)
        assert e.value.code == ife.E_ARG and "set 0" in str(e.value) and list(e.value.n_admissible) == [0]
        assert (to.cpu().numpy()[sl] == 0x5A).all() and _guards_intact(to, sl)
    assert list(ctx.sample_positions(masks[dtype], 0, (71, 1, 1))[1]) == [0]
    assert list(ctx.sample_positions(masks[dtype], 0, (1, 8, 1))[1]) == [0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_and_single_voxels(ctx, dtype):
    """Foreground in the first and last rows only: runs of empty segments share a base, and the
    search must take the last of them.  Then one voxel alone, at either end of the volume."""
    rng = np.random.default_rng(22)
    mask = np.zeros(SHAPE, dtype)
    mask[0, 0] = rng.random(SHAPE[2]) < 0.4
    mask[-1, -1] = rng.random(SHAPE[2]) < 0.4
    mask[0, 0, 0] = mask[-1, -1, -1] = 1
    pos = _check(ctx, mask, N_DRAWS, (1, 1, 1), seed=3)
    assert pos.min() < SHAPE[2] and pos.max() >= mask.size - SHAPE[2]
    mask[0, 0, 64:] = 0      # the partial segment of the first row is empty, the full one not
    mask[-1, -1, :64] = 0    # and the other way round in the last row
    _check(ctx, mask, N_DRAWS, (1, 1, 1), seed=4)
    for where in (0, mask.size - 1, 63, 64, 69, 70):
        mask[...] = 0
        mask.reshape(-1)[where] = 7
        assert (_check(ctx, mask, 9, (1, 1, 1), seed=where)[0] == where).all()


def test_counter_words_seed_and_stream(ctx, masks):
    mask = masks[np.uint8]
    # draws 2^32 - 3 .. 2^32 + 4: the draw number crosses into the second counter word
    pos = _check(ctx, mask, 8, (5, 4, 3), seed=6, first_draw=2 ** 32 - 3)
    assert not np.array_equal(pos[0, 3:], _check(ctx, mask, 5, (5, 4, 3), seed=6, first_draw=0)[0])
    _check(ctx, mask, 8, (5, 4, 3), seed=6, first_draw=2 ** 64 - 3)      # and wraps at 2^64
    # a seed with a high word differs from its low word alone
    hi = _check(ctx, mask, 40, (1, 1, 1), seed=(0xDEADBEEF << 32) | 6)
    assert not np.array_equal(hi, _check(ctx, mask, 40, (1, 1, 1), seed=6))
    # stream 2^32 - 1 and two sets: the second set's stream wraps to 0
    pos = _check(ctx, mask, 40, (1, 1, 1), values=(2, 2), per_value=True, seed=6, stream=2 ** 32 - 1)
    assert np.array_equal(pos[1], _check(ctx, mask, 40, (1, 1, 1), values=(2,), seed=6, stream=0)[0])


def test_draws_are_repeatable_and_splittable(ctx, masks):
    mask = masks[np.uint16]
    kw = dict(size=(5, 4, 3), values=(1, 200), per_value=True, seed=99, stream=1)
    a, _ = ctx.random_rois(mask, 100, **kw)
    b, _ = ctx.random_rois(mask, 100, **kw)
    assert np.array_equal(a, b)
    head, _ = ctx.random_rois(mask, 40, **kw)
    tail, _ = ctx.random_rois(mask, 60, first_draw=40, **kw)
    assert np.array_equal(a, np.concatenate([head, tail], axis=1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_pointer_forms_keep_their_guards(ife, ctx, torch_dev, masks, dtype):
    mask = masks[dtype]
    code = ife.U8 if dtype == np.uint8 else ife.U16
    tm, mptr, msl = _device_bytes(torch_dev, mask.tobytes(), fill=0xFF)   # the guards are foreground
    kw = dict(size=(5, 4, 3), values=(1, 3), per_value=True, seed=12, stream=7, first_draw=5)
    want, counts = S.sample_positions(mask, N_DRAWS, kw["size"], **{k: v for k, v in kw.items() if k != "size"})
    to, optr, sl = _device_bytes(torch_dev, bytes(8 * want.size))
    n = ctx.sample_positions_device(mptr, code, SHAPE, optr, N_DRAWS, **kw)
    assert np.array_equal(n, counts)
    assert np.array_equal(to.cpu().numpy()[sl].view(np.int64).reshape(want.shape), want) and _guards_intact(to, sl)
    to, optr, sl = _device_bytes(torch_dev, bytes(48 * want.size))
    n = ctx.random_rois_device(mptr, code, SHAPE, optr, N_DRAWS, **kw)
    assert np.array_equal(n, counts)
    assert np.array_equal(to.cpu().numpy()[sl].view(np.int64).reshape(want.shape + (6,)),
                          S.boxes_of(want, SHAPE, kw["size"])) and _guards_intact(to, sl)
    # counts alone: no output
    assert np.array_equal(ctx.sample_positions_device(mptr, code, SHAPE, None, 0, **kw), counts)
    # a misaligned output or (uint16) mask pointer
    with pytest.raises(ife.IfeError) as e:
        ctx.sample_positions_device(mptr, code, SHAPE, optr + 4, 1, **kw)
    assert e.value.code == ife.E_ARG
    if dtype == np.uint16:
        with pytest.raises(ife.IfeError) as e:
            ctx.sample_positions_device(mptr + 1, code, SHAPE, optr, 1, **kw)
        assert e.value.code == ife.E_ARG
    assert np.array_equal(tm.cpu().numpy()[msl], np.frombuffer(mask.tobytes(), np.uint8))


def test_more_segments_than_one_scan_chunk(ctx):
    nz, ny, nx = BIG
    assert (nx + 63) // 64 * ny * nz == 4224 > 4096
    rng = np.random.default_rng(23)
    mask = (rng.random(BIG) < 0.3).astype(np.uint8) * rng.integers(1, 4, BIG).astype(np.uint8)
    first_chunk = 4096 // 2 * nx   # the voxels of the first 4096 segments
    assert _check(ctx, mask, 1000, (9, 6, 2), seed=31).max() >= first_chunk   # draws land in the second chunk
    assert _check(ctx, mask, 1000, (1, 1, 1), values=(1, 2, 3), per_value=True, seed=32).max(axis=1).min() >= first_chunk


# ---- extract_rois -------------------------------------------------------------------------------
def _volume(dtype):
    n = int(np.prod(SHAPE))
    if np.dtype(dtype).kind == "f":
        return (np.arange(n, dtype=np.float64) * 1.25 - 7).astype(dtype).reshape(SHAPE)
    return (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << (8 * np.dtype(dtype).itemsize - 1))).astype(dtype).reshape(SHAPE)


def _corner_boxes(size):
    nz, ny, nx = SHAPE
    sx, sy, sz = size
    return [[x, y, z, sx, sy, sz] for z, y, x in itertools.product((0, nz - sz), (0, ny - sy), (0, nx - sx))]


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64])
def test_extract_rois_equals_slicing(ctx, dtype):
    src = _volume(dtype)
    boxes = _corner_boxes((5, 4, 3))
    boxes += [[10, 1, 1, 5, 4, 3], [12, 2, 2, 5, 4, 3], [10, 1, 1, 5, 4, 3], [10, 1, 1, 5, 4, 3]]  # overlapping, repeated
    assert np.array_equal(ctx.extract_rois(src, boxes), S.extract_rois(src, boxes))
    # rows of 67 elements cross the lane seam; x0 = 0 .. 3 and the odd row length put the source
    # and output rows at every byte alignment
    wide = [[x, y, z, 67, 2, 2] for x in range(4) for y in (0, 5) for z in (0, 4)]
    assert np.array_equal(ctx.extract_rois(src, wide), S.extract_rois(src, wide))
    one = [[0, 0, 0, SHAPE[2], SHAPE[1], SHAPE[0]]]
    assert np.array_equal(ctx.extract_rois(src, one)[0], src)
    assert ctx.extract_rois(src, np.empty((0, 6), np.int64)).shape[0] == 0


@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_extract_rois_refusals_leave_dst_untouched(ife, ctx, torch_dev, elem):
    src = _volume({1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}[elem])
    good = [[1, 1, 1, 5, 4, 3], [2, 2, 2, 5, 4, 3]]
    ts, sptr, _ = _device_bytes(torch_dev, src.tobytes())
    for bad in ([66, 1, 1, 5, 4, 3], [1, 4, 1, 5, 4, 3], [1, 1, -1, 5, 4, 3], [1, 1, 1, 5, 4, 2], [1, 1, 1, 5, 0, 3]):
        # the offender last, and first (where its size is the one the others then do not have)
        for boxes in [good + [bad]] + ([[bad] + good] if min(bad[3:]) >= 1 else []):
            with pytest.raises(ife.IfeError) as e:   # checked on the host
                ctx.extract_rois(src, boxes)
            assert e.value.code == ife.E_ARG
            rois = np.array(boxes, np.int64)
            tr, rptr, _ = _device_bytes(torch_dev, rois.tobytes())
            td, dptr, sl = _device_bytes(torch_dev, bytes([0x3C]) * (len(boxes) * 60 * elem))
            with pytest.raises(ife.IfeError) as e:   # checked on the device
                ctx.extract_rois_device(sptr, elem, SHAPE, rptr, len(boxes), dptr)
            assert e.value.code == ife.E_ARG
            assert (td.cpu().numpy()[sl] == 0x3C).all() and _guards_intact(td, sl)
    # n_rois == 0 is legal and writes nothing
    td, dptr, sl = _device_bytes(torch_dev, bytes([0x3C]) * 64)
    ctx.extract_rois_device(sptr, elem, SHAPE, None, 0, dptr)
    assert (td.cpu().numpy()[sl] == 0x3C).all()


@pytest.mark.parametrize("elem,offset", [(1, 1), (1, 3), (2, 2), (4, 4), (8, 8)])
def test_chain_of_device_calls_equals_the_oracle(ife, ctx, torch_dev, masks, elem, offset):
    """random_rois_device -> extract_rois_device, the boxes never leaving the device; the output
    starts `offset` bytes off a 16-byte boundary."""
    dtype = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}[elem]
    src, mask = _volume(dtype), masks[np.uint8]
    size, n = (67, 3, 2), 33
    want_boxes, counts = S.random_rois(mask, n, size, seed=17, stream=3)
    tm, mptr, _ = _device_bytes(torch_dev, mask.tobytes())
    ts, sptr, _ = _device_bytes(torch_dev, src.tobytes())
    tr, rptr, rsl = _device_bytes(torch_dev, bytes(48 * n))
    assert np.array_equal(ctx.random_rois_device(mptr, ife.U8, SHAPE, rptr, n, size=size, seed=17, stream=3), counts)
    td, dptr, sl = _device_bytes(torch_dev, bytes(n * 67 * 3 * 2 * elem), offset=offset)
    assert dptr % 16 == offset % 16
    ctx.extract_rois_device(sptr, elem, SHAPE, rptr, n, dptr)
    got = td.cpu().numpy()[sl].view(dtype).reshape(n, 2, 3, 67)
    assert np.array_equal(got.view(np.uint8), S.extract_rois(src, want_boxes[0]).view(np.uint8)) and _guards_intact(td, sl)
    assert np.array_equal(tr.cpu().numpy()[rsl].view(np.int64).reshape(n, 6), want_boxes[0])
