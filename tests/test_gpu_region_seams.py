"""The seams of region_box_kernel and region_extract_kernel (csrc/region_kernels.hpp) that the
shapes of tests/test_gpu_region.py do not reach: 16-byte pieces that run over several rows and plane
ends, the four-deep steady loop of the box kernel and what stands around it, units of several rows
for 2- and 4-byte elements, and runs of the extract kernel in which a lane takes a second piece.

Everything is integer or bit copying: equality, no tolerance.  The checkers are
tests/region_oracle.py and numpy.  Every test names the constant it crosses and restates the
crossing with the literal number, so that a later change of a shape cannot drop the coverage
unnoticed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_oracle as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
BOX_DTYPES = (np.uint8, np.uint16, np.int16, np.float32)
CODE = {np.uint8: "U8", np.uint16: "U16", np.int16: "I16", np.float32: "F32"}


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


class _DeviceMask:
    """A mask in device memory `offset` bytes behind a 16-byte boundary, between guards that are
    foreground (0xFF bytes: non-zero integers, a NaN), with single elements set and put back."""

    def __init__(self, torch_dev, ife, mask, offset):
        self.torch, self.dev = torch_dev
        self.mask, self.es = mask, mask.dtype.itemsize
        self.code = getattr(ife, CODE[mask.dtype.type])
        self.t, self.ptr, self.where = _device_bytes(torch_dev, mask.tobytes(), offset, fill=0xFF)
        assert self.ptr % 16 == offset

    def box(self, ctx):
        return ctx.mask_bounding_box_device(self.ptr, self.code, self.mask.shape)

    def poke(self, element, value):
        """element (a linear index) = value; returns the bytes that stood there"""
        a = self.where.start + element * self.es
        old = self.t[a:a + self.es].clone()
        new = np.frombuffer(np.array(value, self.mask.dtype).tobytes(), np.uint8).copy()
        self.t[a:a + self.es] = self.torch.from_numpy(new).to(self.dev)
        return old

    def restore(self, element, old):
        a = self.where.start + element * self.es
        self.t[a:a + self.es] = old


def _xyz(element, shape):
    nz, ny, nx = shape
    return element % nx, element // nx % ny, element // (nx * ny)


def _foreground_values(dtype):
    """Non-zero values of the type, used in turn: a zero low byte, the sign bit, a denormal, a NaN."""
    if dtype == np.float32:
        return [np.float32(1e-45), np.float32(np.nan), np.float32(-3.5)]
    if dtype == np.int16:
        return [1, -1, -32768, 256]
    if dtype == np.uint16:
        return [1, 256, 65535]
    return [1, 128, 255]


def _background(shape, dtype):
    """Zeros; for float32 -0.0f, which is background although its bits are not zero."""
    m = np.zeros(shape, dtype)
    if dtype == np.float32:
        m[...] = -0.0
    return m


def _random_mask(shape, dtype, density, rng):
    """Foreground values of the type at about `density` of the voxels, at one voxel at least."""
    on = rng.random(shape) < density
    on.reshape(-1)[rng.integers(on.size)] = True
    m = _background(shape, dtype)
    m[on] = rng.choice(_foreground_values(dtype), int(on.sum()))
    return m


# ---- 1. pieces across rows and planes ------------------------------------------------------------
# csrc/region_kernels.hpp region_box_kernel: a piece holds EPP = 16 / ES elements; where it does not
# lie in one row (x + EPP > nx), `visit` walks it element by element and wraps x, y and z.  With
# nx < EPP a piece runs over several rows, with ny small over several plane ends.
NARROW_SHAPES = [(7, 5, 3), (9, 4, 1), (6, 1, 5), (4, 3, 7), (3, 2, 15)]


def _narrow_shapes(dtype):
    return NARROW_SHAPES + ([(5, 3, 3)] if dtype == np.float32 else [])


def _assert_narrow(shape, dtype):
    """The volume is one unit (far below REGION_BOX_UNIT_BYTES = 16384); aligned, it has at least
    two pieces, and nx below the piece width for uint8."""
    es = np.dtype(dtype).itemsize
    n = int(np.prod(shape))
    assert n * es <= 16384 and n <= 105
    pieces = n * es // 16
    # (6, 1, 5) as uint8 is 30 bytes: one aligned piece (over four plane ends) and 14 tail elements
    assert pieces >= 2 or (shape == (6, 1, 5) and es == 1 and pieces == 1)
    if es == 1:
        assert shape[2] < 16
    if shape == (5, 3, 3):
        assert es == 4 and shape[2] < 16 // 4
    return pieces


@pytest.mark.parametrize("dtype", BOX_DTYPES)
def test_box_pieces_across_rows_and_planes(ctx, dtype):
    rng = np.random.default_rng(61)
    values = _foreground_values(dtype)
    for shape in _narrow_shapes(dtype):
        _assert_narrow(shape, dtype)
        m = _background(shape, dtype)
        flat = m.reshape(-1)
        for e in range(flat.size):
            flat[e] = values[e % len(values)]
            assert ctx.mask_bounding_box(m) == (_xyz(e, shape), (1, 1, 1), 1), (shape, e)
            flat[e] = _background(1, dtype)[0]
        for density in (0.05, 0.5):
            m = _random_mask(shape, dtype, density, rng)
            assert ctx.mask_bounding_box(m) == R.bounding_box(m), (shape, density)


HEAD_OFFSETS = {np.uint8: (1, 2, 3), np.uint16: (2, 4, 6, 8, 10, 12, 14), np.int16: (2, 4, 6, 8, 10, 12, 14),
                np.float32: (4, 8, 12)}


@pytest.mark.parametrize("dtype", BOX_DTYPES)
def test_box_pieces_across_rows_behind_a_head(ife, ctx, torch_dev, dtype):
    """The same volumes through the device form, `offset` bytes behind a 16-byte boundary: a head
    of (16 - offset) / ES elements stands in front of the row-spanning pieces and shifts them."""
    rng = np.random.default_rng(62)
    es = np.dtype(dtype).itemsize
    values = _foreground_values(dtype)
    for shape in _narrow_shapes(dtype):
        _assert_narrow(shape, dtype)
        n = int(np.prod(shape))
        for offset in HEAD_OFFSETS[dtype]:
            head = (16 - offset) // es
            # behind a head the 30 bytes of (6, 1, 5) as uint8 are head and tail alone
            assert 0 < head < 16 // es and ((n - head) * es // 16 >= 1 or (shape == (6, 1, 5) and es == 1))
            dm = _DeviceMask(torch_dev, ife, _background(shape, dtype), offset)
            assert dm.box(ctx) == ((0, 0, 0), (0, 0, 0), 0), (shape, offset)
            for e in range(n):
                old = dm.poke(e, values[e % len(values)])
                assert dm.box(ctx) == (_xyz(e, shape), (1, 1, 1), 1), (shape, offset, e)
                dm.restore(e, old)
            for density in (0.05, 0.5):
                m = _random_mask(shape, dtype, density, rng)
                dm = _DeviceMask(torch_dev, ife, m, offset)
                assert dm.box(ctx) == R.bounding_box(m), (shape, offset, density)


# ---- 2. the steady loop --------------------------------------------------------------------------
# csrc/region_kernels.hpp region_box_kernel: while npieces - p0 >= 4 * REGION_BLOCK = 1024 a lane
# loads four pieces REGION_BLOCK = 256 apart and p0 advances by 1024; the rest goes piece by piece.
# A row longer than REGION_BOX_UNIT_BYTES = 16384 is a unit of its own.
LONG_ROWS = [((2, 3, 40000), np.uint8, 3), ((2, 3, 17000), np.uint16, 6), ((2, 3, 17000), np.int16, 10),
             ((2, 3, 9000), np.float32, 4)]


def _row_layout(ptr_mod16, row, nx, es):
    """(head, npieces, tail0) of a one-row unit, as the kernel computes them"""
    base = ptr_mod16 + row * nx * es
    head = min(nx, ((0 - base) & 15) // es)
    npieces = (nx - head) // (16 // es)
    return head, npieces, head + npieces * (16 // es)


def _steady_elements(ptr_mod16, shape, es):
    """The x of single voxels per row: in the pieces 0, 1023, 1024, 2047, 2048 and the last one (at
    changing places inside the piece), and the first and last element of the head and of the tail
    where the row has them."""
    nz, ny, nx = shape
    epp = 16 // es
    out = []
    for row in (0, 1, ny * nz - 1):
        head, npieces, tail0 = _row_layout(ptr_mod16, row, nx, es)
        assert nx * es > 16384                        # a unit is one row
        assert npieces >= 2 * 1024 + 1                # two steady iterations and a remainder
        assert npieces - 2048 < 1024                  # and no third
        xs = [head + p * epp + (i * 5 + row) % epp for i, p in enumerate((0, 1023, 1024, 2047, 2048, npieces - 1))]
        xs += [head + 1023 * epp + epp - 1, head + 1024 * epp]      # both sides of the loop's seam
        if head:
            xs += [0, head - 1]
        if tail0 < nx:
            xs += [tail0, nx - 1]
        out.append((row, sorted(set(xs))))
    return out


def _long_row_random(shape, dtype, rng):
    m = _background(shape, dtype)
    on = rng.random(shape) < 0.5
    m[on] = rng.choice(_foreground_values(dtype), int(on.sum()))
    m[:, :, :37] = _background(1, dtype)[0]           # the box starts inside the rows
    m[0, 0] = _background(1, dtype)[0]
    return m


@pytest.mark.parametrize("shape,dtype,offset", LONG_ROWS)
def test_box_steady_loop(ctx, shape, dtype, offset):
    """Host form: the staged mask is 16-byte aligned and these rows are whole pieces, so head = 0
    and there is no tail; npieces = 2500, 2125 and 2250."""
    nz, ny, nx = shape
    es = np.dtype(dtype).itemsize
    assert nx * es % 16 == 0 and nx * es // 16 in (2500, 2125, 2250) and nx * es // 16 > 2048
    values = _foreground_values(dtype)
    m = _background(shape, dtype)
    assert ctx.mask_bounding_box(m) == ((0, 0, 0), (0, 0, 0), 0)
    every = []
    for row, xs in _steady_elements(0, shape, es):
        for i, x in enumerate(xs):
            m[row // ny, row % ny, x] = values[i % len(values)]
            assert ctx.mask_bounding_box(m) == ((x, row % ny, row // ny), (1, 1, 1), 1), (row, x)
            m[row // ny, row % ny, x] = _background(1, dtype)[0]
            every.append((row // ny, row % ny, x))
    for z, y, x in every:
        m[z, y, x] = values[x % len(values)]
    assert ctx.mask_bounding_box(m) == R.bounding_box(m)
    assert R.bounding_box(m)[2] == len(every)
    m = _long_row_random(shape, dtype, np.random.default_rng(63))   # dense content: every piece counts
    assert ctx.mask_bounding_box(m) == R.bounding_box(m)


@pytest.mark.parametrize("shape,dtype,offset", LONG_ROWS)
def test_box_steady_loop_behind_a_head(ife, ctx, torch_dev, shape, dtype, offset):
    """Device form, the mask `offset` bytes behind a 16-byte boundary: every row has a head and a
    tail, and the pieces 1023, 1024, 2047 and 2048 hold other elements than in the host form."""
    nz, ny, nx = shape
    es = np.dtype(dtype).itemsize
    for row in range(ny * nz):
        head, npieces, tail0 = _row_layout(offset, row, nx, es)
        assert head == (16 - offset) // es > 0 and tail0 < nx and 2048 < npieces < 3072
    values = _foreground_values(dtype)
    dm = _DeviceMask(torch_dev, ife, _background(shape, dtype), offset)
    assert dm.box(ctx) == ((0, 0, 0), (0, 0, 0), 0)
    for row, xs in _steady_elements(offset, shape, es):
        for i, x in enumerate(xs):
            old = dm.poke(row * nx + x, values[i % len(values)])
            assert dm.box(ctx) == ((x, row % ny, row // ny), (1, 1, 1), 1), (row, x)
            dm.restore(row * nx + x, old)
    m = _long_row_random(shape, dtype, np.random.default_rng(64))
    assert _DeviceMask(torch_dev, ife, m, offset).box(ctx) == R.bounding_box(m)


# ---- 3. units of several rows for 2- and 4-byte elements -----------------------------------------
# csrc/region_capi.inc launch_region_box: REGION_BOX_UNIT_BYTES / row_bytes rows to a unit.
@pytest.mark.parametrize("dtype,per", [(np.uint16, 117), (np.int16, 117), (np.float32, 58)])
def test_box_units_of_several_rows_wide_elements(ctx, dtype, per):
    """Rows of 70 elements: 16384 // 140 = 117 rows to a unit of 2-byte elements, 16384 // 280 = 58
    of float32; 250 rows leave the last unit short (16 and 18 rows).  A unit of 117 * 140 = 16380
    bytes puts the next one 12 bytes behind a 16-byte boundary."""
    es = np.dtype(dtype).itemsize
    shape = (5, 50, 70)
    nrows = 250
    assert 16384 // 140 == 117 and 16384 // 280 == 58 and per == 16384 // (70 * es)
    assert nrows % per in (16, 18) and nrows // per >= 2
    values = _foreground_values(dtype)
    m = _background(shape, dtype)
    flat = m.reshape(nrows, 70)
    rows = [r for u in range(1, nrows // per + 1) for r in (u * per - 1, u * per)] + [nrows - 1]
    assert all(0 <= r < nrows for r in rows)
    for i, row in enumerate(rows):
        for x in (0, 69):
            flat[row, x] = values[i % len(values)]
            assert ctx.mask_bounding_box(m) == ((x, row % 50, row // 50), (1, 1, 1), 1), (row, x)
            flat[row, x] = _background(1, dtype)[0]
    for i, row in enumerate(rows):
        flat[row, 0 if i % 2 else 69] = values[i % len(values)]
    assert ctx.mask_bounding_box(m) == R.bounding_box(m) and R.bounding_box(m)[2] == len(rows)
    m = _background(shape, dtype)
    on = np.random.default_rng(65).random(shape) < 0.3
    m[on] = values[0]
    m[:, :3] = _background(1, dtype)[0]
    assert ctx.mask_bounding_box(m) == R.bounding_box(m)


# ---- 4. extract: every run longer than one wave trip --------------------------------------------
# csrc/region_kernels.hpp region_extract_kernel: a wave takes an output row, and each of its four
# piece loops (pad low, copy, copy with FLIPX, pad high) strides by the 64 lanes.
ELEM_DTYPES = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}


def _source(es):
    """The `sources` recipe of tests/test_gpu_region.py: every byte differs from its neighbours,
    and a pad value whose bytes all differ."""
    epp = 16 // es
    shape = (2, 3, 66 * epp + 5)
    dt = ELEM_DTYPES[es]
    raw = np.random.default_rng(11 + es).integers(1, 250, shape + (es,), dtype=np.uint8)
    pad = np.frombuffer(bytes(range(0xF1, 0xF1 + es)), dt)[0]
    return np.ascontiguousarray(raw).view(dt).reshape(shape), pad


def _runs(dst_mod16, row, sx, lo, n, es):
    """(head, nb, k1, k2, k3, k4) of an output row: the kernel's arithmetic restated"""
    epp = 16 // es
    head = min(sx, ((0 - (dst_mod16 + row * sx * es)) & 15) // es)
    nb = (sx - head) // epp
    a, b = lo - head, lo + n - head
    k1, k2 = (0, 0) if a <= 0 else (a // epp, (a + epp - 1) // epp)
    k3, k4 = (0, 0) if b <= 0 else (b // epp, (b + epp - 1) // epp)
    k1, k2 = min(k1, nb), min(k2, nb)
    k3 = min(max(k3, k2), nb)
    k4 = min(max(k4, k3), nb)
    return head, nb, k1, k2, k3, k4


def _long_regions(epp):
    """(index, size) of two regions over a source row of 66 * EPP + 5 elements.  The first has 65 *
    EPP + 3 elements of pad in front and 64 * EPP + 3 behind; its high pad has 63 or more whole
    pieces (63 for one-byte elements at an aligned row) and, flipped along x, its low pad 64.  The
    second has 67 * EPP + 3 on both sides: more than 64 whole pieces in every run, at every
    alignment, flipped or not.  y: one row of pad in front, whose low pad run is the whole row."""
    return [((-(65 * epp + 3), -1, 0), (3 * 65 * epp + 11, 4, 2)),
            ((-(67 * epp + 3), -1, 0), (2 * (67 * epp + 3) + 66 * epp + 5, 4, 2))]


EXTRACT_FLIPS = [(False, False, False), (True, False, False), (False, True, False), (True, False, True)]


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_extract_runs_longer_than_a_wave_trip(ife, ctx, torch_dev, es):
    torch, _ = torch_dev
    epp = 16 // es
    src, pad = _source(es)
    nx = src.shape[2]
    s_t, s_ptr, _ = _device_bytes(torch_dev, src.tobytes())
    for which, (index, size) in enumerate(_long_regions(epp)):
        sx = size[0]
        for flip in EXTRACT_FLIPS:
            lo, n, hi, _, _ = R.axis_split(index[0], sx, nx, flip[0])
            assert n == nx == 66 * epp + 5
            want = R.extract_region(src, index, size, pad, flip)
            # host to host: the staged output is aligned, row 0 has no head
            head, nb, k1, k2, k3, k4 = _runs(0, 0, sx, lo, n, es)
            assert head == 0 and k3 - k2 > 64 and k1 >= 64 and nb - k4 >= 63
            if which == 1:
                assert k1 > 64 and k3 - k2 > 64 and nb - k4 > 64
            elif not flip[0]:
                assert k1 > 64
            got = ctx.extract_region(src, index, size, pad_value=pad, flip=flip)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (index, size, flip)
            # device to device at every element-aligned offset of dst inside 16 bytes
            for offset in range(0, 16, es):
                if which == 1:
                    for row in range(size[1] * size[2]):
                        head, nb, k1, k2, k3, k4 = _runs(offset, row, sx, lo, n, es)
                        assert k1 > 64 and k3 - k2 > 64 and nb - k4 > 64
                d_t, d_ptr, where = _device_bytes(torch_dev, bytes(want.nbytes), offset)
                assert d_ptr % 16 == offset
                ctx.extract_region_device(s_ptr, es, src.shape, index, size, d_ptr, pad_value=pad.tobytes(), flip=flip)
                torch.cuda.synchronize()
                back = d_t.cpu().numpy()
                assert back[where].tobytes() == want.tobytes(), (index, size, flip, offset)
                assert (back[:where.start] == 0xA5).all() and (back[where.stop:] == 0xA5).all(), (flip, offset)
    assert (s_t.cpu().numpy()[:GUARD] == 0xA5).all()
