"""The region calls on the device (ife_mask_bounding_box, ife_extract_region,
ife_label_membership) against tests/region_oracle.py.  Nothing here has a tolerance: boxes, counts
and copied bits are compared for equality.  The shapes are the smallest that reach every path: a
row of 70 elements crosses the 64-lane seam and is no multiple of 16 bytes, so that rows start at
every byte alignment and every run has a head, aligned pieces and a tail."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_oracle as R  # noqa: E402

pytestmark = pytest.mark.gpu

BOX_SHAPE = (6, 7, 70)
BOX_DTYPES = (np.uint8, np.uint16, np.int16, np.float32)
GUARD = 64


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


# ---- bounding box ------------------------------------------------------------------------------
def _check_box(ctx, mask):
    assert ctx.mask_bounding_box(mask) == R.bounding_box(mask)


@pytest.mark.parametrize("shape", [BOX_SHAPE, (3, 5, 1)])
@pytest.mark.parametrize("dtype", BOX_DTYPES)
def test_box_empty_full_corners_and_sparse(ctx, shape, dtype):
    nz, ny, nx = shape
    m = np.zeros(shape, dtype)
    assert ctx.mask_bounding_box(m) == ((0, 0, 0), (0, 0, 0), 0)
    full = np.ones(shape, dtype)
    assert ctx.mask_bounding_box(full) == ((0, 0, 0), (nx, ny, nz), nx * ny * nz)
    corners = list(itertools.product((0, nz - 1), (0, ny - 1), (0, nx - 1)))
    for z, y, x in corners + [(nz // 2, ny // 2, nx // 2)]:
        m[...] = 0
        m[z, y, x] = 3
        assert ctx.mask_bounding_box(m) == ((x, y, z), (1, 1, 1), 1)
    m[...] = 0
    m[0, 0, 0] = m[-1, -1, -1] = 1   # two opposite corners (one voxel where the shape has one corner)
    _check_box(ctx, m)
    m[...] = 0
    m[0, -1, 0] = m[-1, 0, -1] = 1
    _check_box(ctx, m)
    rng = np.random.default_rng(7)
    for density in (0.004, 0.05, 0.5):
        m = (rng.random(shape) < density).astype(dtype) * 5
        _check_box(ctx, m)
        m[:, :, : nx // 3] = 0   # the box starts inside a row
        m[: nz // 2] = 0
        _check_box(ctx, m)


def test_box_every_x_of_a_row(ctx):
    """One voxel at every x of one row: every lane and every head, piece and tail position."""
    for dtype in (np.uint8, np.float32):
        m = np.zeros(BOX_SHAPE, dtype)
        for x in range(BOX_SHAPE[2]):
            m[...] = 0
            m[3, 5, x] = 1
            assert ctx.mask_bounding_box(m) == ((x, 5, 3), (1, 1, 1), 1)


def test_box_foreground_rules(ctx):
    u = np.zeros(BOX_SHAPE, np.uint16)
    u[2, 3, 40] = 256   # low byte zero
    assert ctx.mask_bounding_box(u) == ((40, 3, 2), (1, 1, 1), 1)
    i = np.zeros(BOX_SHAPE, np.int16)
    i[1, 2, 3] = -1
    i[4, 6, 69] = -32768
    assert ctx.mask_bounding_box(i) == R.bounding_box(i) == ((3, 2, 1), (67, 5, 4), 2)
    f = np.zeros(BOX_SHAPE, np.float32)
    f[:] = -0.0          # background, although its bits are not zero
    assert ctx.mask_bounding_box(f) == ((0, 0, 0), (0, 0, 0), 0)
    f[1, 1, 17] = np.float32(1e-45)   # the smallest denormal
    f[5, 2, 66] = np.nan
    assert ctx.mask_bounding_box(f) == R.bounding_box(f) == ((17, 1, 1), (50, 2, 5), 2)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_box_uint8_device_pointer_at_odd_offsets(ife, ctx, torch_dev, offset):
    rng = np.random.default_rng(offset)
    m = (rng.random(BOX_SHAPE) < 0.03).astype(np.uint8)
    m[:, :2] = 0
    t, ptr, _ = _device_bytes(torch_dev, m.tobytes(), offset, fill=0xFF)   # the guards are foreground
    assert ptr % 4 == offset
    assert ctx.mask_bounding_box_device(ptr, ife.U8, m.shape) == R.bounding_box(m)


def test_box_more_units_than_the_grid_cap(ctx):
    """csrc/region_kernels.hpp: a workgroup takes units of whole rows of REGION_BOX_UNIT_BYTES =
    16384 bytes, one row where a row is longer, and the grid holds at most REGION_BOX_GRID_CAP =
    2048 workgroups.  Rows of 16400 bytes are units of their own, 2100 of them are more than the
    cap; the only voxel lies in the last row."""
    nz, ny, nx = 3, 700, 16400
    assert nx > 16384 and nz * ny == 2100 > 2048
    m = np.zeros((nz, ny, nx), np.uint8)
    m[-1, -1, 12345] = 1
    assert ctx.mask_bounding_box(m) == ((12345, ny - 1, nz - 1), (1, 1, 1), 1)
    m[0, 0, 16399] = 1
    assert ctx.mask_bounding_box(m) == ((12345, 0, 0), (16399 - 12345 + 1, ny, nz), 2)


def test_box_units_of_several_rows(ctx):
    """Rows of 70 bytes: 16384 // 70 = 234 rows to a unit, 1000 rows are five units, the last
    one short; one voxel per unit seam."""
    assert 16384 // 70 == 234
    m = np.zeros((10, 100, 70), np.uint8)
    flat = m.reshape(1000, 70)
    for row in (233, 234, 467, 468, 999):
        flat[...] = 0
        flat[row, 69] = 1
        assert ctx.mask_bounding_box(m) == ((69, row % 100, row // 100), (1, 1, 1), 1)
    flat[...] = 0
    flat[233, 3] = flat[936, 60] = 1
    _check_box(ctx, m)


# ---- extract -----------------------------------------------------------------------------------
SRC_SHAPE = (5, 6, 70)
ELEM_DTYPES = (np.uint8, np.int16, np.float32, np.float64)


@pytest.fixture(scope="module")
def sources():
    """One source per element size whose bytes all differ from their neighbours', and a pad value
    whose bytes all differ."""
    rng = np.random.default_rng(11)
    out = {}
    for dt in ELEM_DTYPES:
        es = np.dtype(dt).itemsize
        raw = rng.integers(1, 250, SRC_SHAPE + (es,), dtype=np.uint8)
        pad = np.frombuffer(bytes(range(0xF1, 0xF1 + es)), dt)[0]
        out[dt] = (np.ascontiguousarray(raw).view(dt).reshape(SRC_SHAPE), pad)
    return out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", ELEM_DTYPES)
def test_extract_inside_regions_at_every_source_offset(ctx, sources, dtype):
    src, _ = sources[dtype]
    for ix in range(18):
        for sx in (1, 15, 16, 17, 37):
            got = ctx.extract_region(src, (ix, 1, 2), (sx, 4, 2))
            assert _same_bits(got, R.extract_region(src, (ix, 1, 2), (sx, 4, 2))), (ix, sx)
    nz, ny, nx = SRC_SHAPE
    assert _same_bits(ctx.extract_region(src, (0, 0, 0), (nx, ny, nz)), src)
    assert _same_bits(ctx.extract_region(src, (69, 5, 4), (1, 1, 1)), src[4:, 5:, 69:])


@pytest.mark.parametrize("dtype", ELEM_DTYPES)
def test_extract_pads_every_side_and_wholly_outside(ctx, sources, dtype):
    src, pad = sources[dtype]
    nz, ny, nx = SRC_SHAPE
    cases = [((-3, 0, 0), (20, ny, nz)), ((60, 0, 0), (33, ny, nz)),        # x low, x high
             ((0, -2, 0), (nx, 5, nz)), ((0, 4, 0), (nx, 5, nz)),           # y
             ((0, 0, -1), (nx, ny, 3)), ((0, 0, 3), (nx, ny, 4)),           # z
             ((-5, -2, -1), (nx + 9, ny + 3, nz + 3)),                      # every side at once
             ((-1, 2, 1), (3, 1, 1)), ((68, 2, 1), (19, 2, 1)),             # a copy run inside one piece
             ((nx, 0, 0), (5, 2, 2)), ((0, -4, 0), (7, 4, 2)), ((3, 3, nz + 2), (37, 2, 2)),   # wholly outside
             ((-40, 1, 1), (17, 2, 2))]
    for index, size in cases:
        got = ctx.extract_region(src, index, size, pad_value=pad)
        assert _same_bits(got, R.extract_region(src, index, size, pad)), (index, size)


@pytest.mark.parametrize("dtype", ELEM_DTYPES)
def test_extract_all_eight_flips(ctx, sources, dtype):
    src, pad = sources[dtype]
    for flip in itertools.product((False, True), repeat=3):
        for index, size in (((2, 1, 1), (37, 4, 3)), ((0, 0, 0), SRC_SHAPE[::-1]), ((-3, -1, 2), (21, 4, 5)),
                            ((55, 3, -1), (33, 5, 3)), ((7, 0, 0), (1, 6, 1)), ((1, 2, 3), (16, 1, 1))):
            got = ctx.extract_region(src, index, size, pad_value=pad, flip=flip)
            assert _same_bits(got, R.extract_region(src, index, size, pad, flip)), (flip, index, size)
    # flip as the header's bits: bit a flips axis a
    got = ctx.extract_region(src, (2, 1, 1), (37, 4, 3), flip=5)
    assert _same_bits(got, R.extract_region(src, (2, 1, 1), (37, 4, 3), None, (True, False, True)))


def test_constant_pad_filter_as_a_region(ctx, sources):
    src, pad = sources[np.int16]
    nz, ny, nx = SRC_SHAPE
    got = ctx.extract_region(src, (-4, -1, 0), (nx + 4 + 5, ny + 1 + 2, nz), pad_value=pad)
    assert _same_bits(got, np.pad(src, ((0, 0), (1, 2), (4, 5)), constant_values=pad))


@pytest.mark.parametrize("dtype", ELEM_DTYPES)
def test_extract_device_to_device_with_guards(ife, ctx, torch_dev, sources, dtype):
    """dst at every element-aligned offset inside 16 bytes (odd byte offsets for one-byte
    elements); the 64 guard bytes before and after stay untouched."""
    torch, _ = torch_dev
    src, pad = sources[dtype]
    es = src.dtype.itemsize
    s_t, s_ptr, _ = _device_bytes(torch_dev, src.tobytes())
    for offset in range(0, 16, es):
        for index, size, flip in (((3, 1, 1), (37, 3, 2), (False, False, False)),
                                  ((-2, -1, 0), (23, 4, 2), (True, False, True))):
            want = R.extract_region(src, index, size, pad, flip)
            d_t, d_ptr, where = _device_bytes(torch_dev, bytes(want.nbytes), offset)
            ctx.extract_region_device(s_ptr, es, src.shape, index, size, d_ptr, pad_value=pad.tobytes(), flip=flip)
            torch.cuda.synchronize()
            back = d_t.cpu().numpy()
            assert back[where].tobytes() == want.tobytes(), (offset, index)
            assert (back[:where.start] == 0xA5).all() and (back[where.stop:] == 0xA5).all(), (offset, index)
    assert (s_t.cpu().numpy()[:GUARD] == 0xA5).all()


def test_extract_mixed_memory_modes(ife, ctx, torch_dev, sources):
    """A volume uploaded once serves fetches to the host (ExtractSlices); and the reverse."""
    torch, _ = torch_dev
    src, pad = sources[np.float32]
    lib = ife.load_library()
    d = ife._desc(src.shape, (1.0, 1.0, 1.0))
    s_t, s_ptr, _ = _device_bytes(torch_dev, src.tobytes())
    for axis in range(3):
        size = list(SRC_SHAPE[::-1])
        size[axis] = 1
        index = [0, 0, 0]
        index[axis] = 2
        region = (C.c_int64 * 6)(*(index + size))
        out = np.empty(size[::-1], np.float32)
        ctx._chk(lib.ife_extract_region(ctx._h, C.c_void_p(s_ptr), 4, C.byref(d), region, 4 if axis < 2 else 0, None,
                                        out.ctypes.data, ife.MEM_DEVICE, ife.MEM_HOST))
        assert _same_bits(out, R.extract_region(src, index, size, None, (False, False, axis < 2)))
    index, size = (-1, 2, 1), (40, 3, 3)
    want = R.extract_region(src, index, size, pad)
    d_t, d_ptr, where = _device_bytes(torch_dev, bytes(want.nbytes), 4)
    region = (C.c_int64 * 6)(*(index + size))
    ctx._chk(lib.ife_extract_region(ctx._h, src.ctypes.data, 4, C.byref(d), region, 0, pad.tobytes(),
                                    C.c_void_p(d_ptr), ife.MEM_HOST, ife.MEM_DEVICE))
    torch.cuda.synchronize()
    back = d_t.cpu().numpy()
    assert back[where].tobytes() == want.tobytes()
    assert (back[:where.start] == 0xA5).all() and (back[where.stop:] == 0xA5).all()


def test_extract_more_rows_than_the_grid_cap(ctx):
    """csrc/region_kernels.hpp: a wave takes an output row, a workgroup four, and the grid holds
    at most REGION_EXTRACT_GRID_CAP = 4096 workgroups: 130 * 130 = 16900 rows are more than the
    4 * 4096 = 16384 of one trip."""
    assert 130 * 130 == 16900 > 4 * 4096
    rng = np.random.default_rng(5)
    src = rng.integers(0, 2 ** 16, (131, 132, 9), dtype=np.uint16)
    for flip in ((False, False, False), (True, True, True)):
        got = ctx.extract_region(src, (4, 1, 1), (3, 130, 130), flip=flip)
        assert _same_bits(got, R.extract_region(src, (4, 1, 1), (3, 130, 130), None, flip))


def test_extract_refusals_on_the_device(ife, ctx, torch_dev, sources):
    src, pad = sources[np.float32]
    lib = ife.load_library()
    d = ife._desc(src.shape, (1.0, 1.0, 1.0))
    out = np.full(8, 7.0, np.float32)
    nbytes = src.nbytes

    def call(region, flip=0, pad_value=None, elem_bytes=4, src_ptr=src.ctypes.data, dst_ptr=out.ctypes.data,
             src_mem=ife.MEM_HOST, dst_mem=ife.MEM_HOST):
        return lib.ife_extract_region(ctx._h, C.c_void_p(src_ptr), elem_bytes, C.byref(d), (C.c_int64 * 6)(*region),
                                      flip, pad_value, C.c_void_p(dst_ptr), src_mem, dst_mem)

    assert call((0, 0, 0, 2, 2, 2), elem_bytes=3) == ife.E_ARG
    assert call((0, 0, 0, 2, 0, 2)) == ife.E_ARG
    assert call((0, 0, 0, 2, 2, 2), flip=8) == ife.E_ARG
    assert call((-1, 0, 0, 2, 2, 2)) == ife.E_ARG                      # reaches outside, NULL pad value
    assert call((0, 0, 0, 2 ** 20, 2 ** 20, 2), pad_value=pad.tobytes()) == ife.E_SIZE
    assert call((0, 0, 0, 2 ** 62, 2 ** 62, 2 ** 62), pad_value=pad.tobytes()) == ife.E_SIZE
    assert (out == 7.0).all()
    t, ptr, _ = _device_bytes(torch_dev, src.tobytes())
    dev = dict(src_ptr=ptr, src_mem=ife.MEM_DEVICE, dst_mem=ife.MEM_DEVICE)
    assert call((0, 0, 0, 2, 2, 2), dst_ptr=ptr + nbytes - 4, **dev) == ife.E_ARG     # overlap
    assert call((0, 0, 0, 2, 2, 2), dst_ptr=ptr + 2, **dev) == ife.E_ARG              # and misaligned
    assert call((0, 0, 0, 2, 2, 2), dst_ptr=ptr + nbytes + 2, **dev) == ife.E_ARG     # misaligned only
    assert t.cpu().numpy()[GUARD:GUARD + nbytes].tobytes() == src.tobytes()


# ---- membership --------------------------------------------------------------------------------
SETS = {np.uint8: [[0], [255], [7, 3, 7, 200, 3], []],
        np.uint16: [[0], [65535], [255, 256], [900, 3, 900, 65535, 256, 3], []]}


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
def test_membership_sets_and_extremes(ctx, dtype, n):
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(n)
    pool = np.array([0, 1, 3, 7, 200, 255] + ([256, 257, 900, 65534, 65535] if dtype == np.uint16 else []), dtype)
    lab = rng.choice(pool, n).astype(dtype)
    lab[-1] = top
    for include in SETS[dtype]:
        for inside, outside in ((1, 0), (top, 0), (0, top), (top, top), (5, 5)):
            got = ctx.label_membership(lab, include, inside, outside)
            assert _same_bits(got, R.label_membership(lab, include, inside, outside)), (include, inside, outside)
    assert (ctx.label_membership(lab, [], 1, 0) == 0).all()
    vol = rng.choice(pool, (3, 5, 7)).astype(dtype)   # the shape is kept
    assert _same_bits(ctx.label_membership(vol, [3, 255]), R.label_membership(vol, [3, 255]))


@pytest.mark.parametrize("dtype,code", [(np.uint8, "U8"), (np.uint16, "U16")])
def test_membership_device_pointers_and_guards(ife, ctx, torch_dev, dtype, code):
    torch, _ = torch_dev
    es = np.dtype(dtype).itemsize
    rng = np.random.default_rng(3)
    for n in (1, 15, 16, 17, 4099):
        lab = rng.integers(0, 12, n).astype(dtype)
        want = R.label_membership(lab, [11, 2, 5], 9, 4)
        for in_off, out_off in ((0, 0), (es, 3 * es), (5 * es, 2 * es)):   # the two alignments differ
            l_t, l_ptr, _ = _device_bytes(torch_dev, lab.tobytes(), in_off)
            o_t, o_ptr, where = _device_bytes(torch_dev, bytes(want.nbytes), out_off)
            ctx.label_membership_device(l_ptr, getattr(ife, code), n, [11, 2, 5], o_ptr, inside=9, outside=4)
            torch.cuda.synchronize()
            back = o_t.cpu().numpy()
            assert back[where].tobytes() == want.tobytes(), (n, in_off, out_off)
            assert (back[:where.start] == 0xA5).all() and (back[where.stop:] == 0xA5).all(), (n, in_off, out_off)


def test_membership_more_pieces_than_one_trip(ctx):
    """csrc/region_kernels.hpp: REGION_MEMBER_GRID_CAP = 2048 workgroups of 256 lanes take 524288
    pieces of 16 bytes in a trip; 8.4 million uint8 labels are more."""
    n = 16 * 2048 * 256 + 4099
    assert n // 16 > 2048 * 256
    rng = np.random.default_rng(9)
    lab = rng.integers(0, 256, n).astype(np.uint8)
    got = ctx.label_membership(lab, [0, 17, 255], 200, 3)
    assert _same_bits(got, R.label_membership(lab, [0, 17, 255], 200, 3))


def test_membership_refusals_on_the_device(ife, ctx):
    lib = ife.load_library()
    lab = np.zeros(8, np.uint8)
    out = np.full(8, 9, np.uint8)

    def call(include, inside=1, outside=0, n=8, dtype=ife.U8):
        inc = (C.c_int * max(len(include), 1))(*include)
        return lib.ife_label_membership(ctx._h, lab.ctypes.data, dtype, n, inc, len(include), inside, outside,
                                        out.ctypes.data, ife.MEM_HOST)

    assert call([256]) == ife.E_ARG and call([-1]) == ife.E_ARG
    assert call([1], inside=256) == ife.E_ARG and call([1], outside=-1) == ife.E_ARG
    assert call([1], dtype=ife.F32) == ife.E_ARG
    assert call([1], n=0) == ife.E_SIZE
    assert (out == 9).all()
    assert call([65535], n=4, dtype=ife.U16) == ife.OK


# ---- chain -------------------------------------------------------------------------------------
def test_chain_box_then_crop_on_the_device(ife, ctx, torch_dev, synth):
    """The bounding box of a device mask, then the crop of a device image to it, with no copy of
    either volume in between: equal to the host calls."""
    torch, dev = torch_dev
    shape = (20, 33, 70)
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    index, size, count = ctx.mask_bounding_box(mask)
    assert (index, size, count) == R.bounding_box(mask) and 0 < count < mask.size
    want = ctx.extract_region(img, index, size)
    assert _same_bits(want, R.extract_region(img, index, size))
    d_img, d_mask = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    torch.cuda.synchronize()
    got_box = ctx.mask_bounding_box_device(d_mask.data_ptr(), ife.U8, shape)
    assert got_box == (index, size, count)
    d_out = torch.full(tuple(size[::-1]), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.extract_region_device(d_img.data_ptr(), 4, shape, got_box[0], got_box[1], d_out.data_ptr())
    torch.cuda.synchronize()
    assert _same_bits(d_out.cpu().numpy(), want)
