"""ife_bspline_coefficients*, ife_resample_bspline* and ife_window_u8 on the device against the numpy
oracle (tests/bspline_oracle.py), bit for bit in every case: the host tables are the same IEEE
operations in C++ and in numpy (tests/test_bspline_plan_cpu.py), and the sweeps and nested sums
round every operation on its own on the device (-ffp-contract=off) as numpy does.  Floats are
compared as integers; sources are finite.

Each order's shapes put its poles' boundaries between the full causal start and the truncated one
(N = h and N = h + 1) and the two-sample line on every axis.  The line passes, the conversion and
the window cap their grids at 2048 workgroups of 256 and the gather at 2^12 workgroups, each of
one output y and eight output planes; the *_beyond_the_*_cap tests take the second trip of each
loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bspline_oracle as B  # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS = (0, 1, 2, 3, 4, 5)
BOUNDARY = {2: [(15, 14, 2), (2, 15, 14), (14, 2, 15)],
            3: [(19, 18, 2), (2, 19, 18), (18, 2, 19)],
            4: [(24, 23, 7), (6, 24, 23), (23, 2, 24)],
            5: [(29, 28, 9), (8, 29, 28), (28, 2, 29)]}
SECOND_POLE = {4: [(7, 6, 2), (2, 7, 6), (6, 2, 7)], 5: [(9, 8, 2), (2, 9, 8), (8, 2, 9)]}
OTHER = [(1, 9, 29), (3, 5, 300), (7, 70, 33)]
DTYPES = {"f32": np.float32, "i16": np.int16, "u8": np.uint8, "u16": np.uint16, "f64": np.float64}
LINE_CAP = 2048 * 256

# the general geometry of tests/test_gpu_resample.py: part of every axis of the output lies outside
G_SRC = dict(shape=(5, 9, 70), spacing=(0.7, 0.7, 2.5), origin=(-100.3, 5.0, -7.0))
G_DST = dict(shape=(21, 13, 67), spacing=(0.9, 0.55, 0.625), origin=(-98.1, 4.1, -8.0))
G_T = (0.4, 0.0, 0.2)
G_GEOM = (G_SRC["spacing"], G_SRC["origin"], G_DST["shape"], G_DST["spacing"], G_DST["origin"])


def _source(shape, dtype=np.float64, seed=1):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)
    return (rng.standard_normal(shape) * 1000).astype(dtype)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(B.bits(got).ravel() != B.bits(want).ravel())
    assert bad.size == 0, "%s: %d values differ, first at %d: %r != %r" % (
        what, bad.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


# ---- coefficients -------------------------------------------------------------------------------

@pytest.mark.parametrize("order", sorted(BOUNDARY))
def test_coefficients_at_the_boundary_lengths(ctx, order):
    # what the shapes are chosen for: N = h and N = h + 1 of every pole on every axis (the first
    # three shapes of an order do that for its first pole and put the second pole's pair on one
    # axis each; SECOND_POLE completes the second pole's)
    shapes = BOUNDARY[order] + SECOND_POLE.get(order, [])
    for z, h in zip(B.poles(order), B.HORIZONS[order]):
        assert B.start_table(z, h, h)[0] and not B.start_table(z, h, h + 1)[0]
        for axis in range(3):
            assert {h, h + 1} <= {s[axis] for s in shapes}
    for shape in shapes:
        src = _source(shape, seed=order)
        _same(ctx.bspline_coefficients(src, order), B.coefficients(src, order), "order %d %r" % (order, shape))
    assert all(any(s[axis] == 2 for s in shapes) for axis in range(3))     # the two-sample line


@pytest.mark.parametrize("shape", OTHER, ids=["length_one_axis", "long_x_odd_count", "more_than_a_workgroup"])
@pytest.mark.parametrize("order", ORDERS)
def test_coefficients_on_other_lines(ctx, order, shape):
    src = _source(shape, seed=10 + order)
    _same(ctx.bspline_coefficients(src, order), B.coefficients(src, order), "order %d %r" % (order, shape))


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_coefficients_of_every_source_type(ctx, name):
    src = _source((7, 70, 33), DTYPES[name], seed=3)
    for order in (1, 3, 4):
        _same(ctx.bspline_coefficients(src, order), B.coefficients(src, order), "%s order %d" % (name, order))


def test_coefficients_in_place_equal_out_of_place(ctx):
    import torch
    dev = torch.device("cuda", 0)
    src = _source((23, 2, 24), seed=4)
    for order in (3, 4):
        want = B.coefficients(src, order)
        d_src = torch.from_numpy(src).to(dev)
        d_out = torch.zeros_like(d_src)
        torch.cuda.synchronize()
        ctx.bspline_coefficients_device(d_src.data_ptr(), None, src.shape, order, d_out.data_ptr())
        ctx.synchronize()
        assert np.array_equal(d_src.cpu().numpy(), src)                      # the source is left alone
        ctx.bspline_coefficients_device(d_src.data_ptr(), None, src.shape, order, d_src.data_ptr())
        ctx.synchronize()
        _same(d_out.cpu().numpy(), want, "out of place, order %d" % order)
        _same(d_src.cpu().numpy(), want, "in place, order %d" % order)


@pytest.mark.parametrize("shape", [(2, 513, 1024), (1024, 2, 513), (513, 1024, 2)], ids=["z_lines", "y_lines", "x_rows"])
def test_lines_beyond_the_grid_cap(ctx, shape):
    """more than 2048 * 256 lines along one axis (and as many values to convert): the lanes of the
    capped grid take a second line"""
    nz, ny, nx = shape
    assert max(nx * ny, nx * nz, ny * nz) > LINE_CAP
    src = _source(shape, np.float32, seed=5)
    _same(ctx.bspline_coefficients(src, 3), B.coefficients(src, 3), repr(shape))


# ---- resampling ---------------------------------------------------------------------------------

def _inside(order, src_shape, geom, translation):
    tx, ty, tz = B.tables(order, src_shape, geom[0], geom[1], geom[2], geom[3], geom[4], translation)
    return tz[0][:, None, None] & ty[0][None, :, None] & tx[0][None, None, :]


@pytest.mark.parametrize("name", ["f32", "f64"])
@pytest.mark.parametrize("extrapolate", [False, True], ids=["default", "nearest"])
@pytest.mark.parametrize("order", ORDERS)
def test_general_geometry(ctx, order, extrapolate, name):
    src = _source(G_SRC["shape"], DTYPES[name], seed=6)
    want = B.resample(src, *G_GEOM, G_T, order, extrapolate, -7.5)
    got = ctx.resample_bspline(src, *G_GEOM, translation=G_T, order=order, extrapolate=extrapolate, default=-7.5)
    assert got.dtype == DTYPES[name]
    _same(got, want, "order %d" % order)
    inside = _inside(order, src.shape, G_GEOM, G_T)
    if extrapolate:
        assert not (got == -7.5).any()
        assert np.isin(got[~inside], src).all()              # outside voxels are source voxels
        assert got[20, 0, 66] == src[4, 0, 69] and got[0, 0, 66] == src[0, 0, 69]   # the far x edge, low y
    else:
        assert abs((got == -7.5).mean() - 0.375) < 0.01      # a forgotten default cannot pass on zeros
        assert ((got == -7.5) == ~inside).all()


@pytest.mark.parametrize("name", ["i16", "u8", "u16"])
def test_general_geometry_integer_sources(ctx, name):
    src = _source(G_SRC["shape"], DTYPES[name], seed=7)
    for order, extrapolate in ((3, True), (2, False)):
        want = B.resample(src, *G_GEOM, G_T, order, extrapolate, -7.5)
        got = ctx.resample_bspline(src, *G_GEOM, translation=G_T, order=order, extrapolate=extrapolate, default=-7.5)
        _same(got, want, "%s order %d" % (name, order))


@pytest.mark.parametrize("order", ORDERS)
def test_a_source_of_one_plane(ctx, order):
    """nz = 1: the z axis is absent, one tap of weight one"""
    src = _source((1, 9, 70), seed=8)
    geom = (G_SRC["spacing"], G_SRC["origin"], (3, 13, 67), G_DST["spacing"], (G_DST["origin"][0], 4.1, -7.5))
    for extrapolate in (False, True):
        want = B.resample(src, *geom, G_T, order, extrapolate, -7.5)
        got = ctx.resample_bspline(src, *geom, translation=G_T, order=order, extrapolate=extrapolate, default=-7.5)
        _same(got, want, "order %d" % order)
    flat = B.resample(src[0][None], *geom, G_T, order, True, -7.5)
    assert np.array_equal(flat[0], flat[1]) and np.array_equal(flat[0], flat[2])       # as a 2-D image


def test_rows_beyond_the_gather_cap(ctx):
    """256 output rows times 33 groups of eight planes, more than 2^12 workgroups: those of the
    capped grid take a second and a third group; the last group of a column has one plane"""
    src = _source((9, 8, 3), np.float32, seed=9)
    d_shape = (257, 256, 3)
    assert d_shape[1] * ((d_shape[0] + 7) // 8) > 2 * (1 << 12) and d_shape[0] % 8 == 1
    geom = ((1.0, 1.0, 1.0), (0, 0, 0), d_shape, (0.9, 8.0 / 256, 9.5 / 257), (-0.3, -0.2, -0.4))
    for order in (3, 4):
        _same(ctx.resample_bspline(src, *geom, order=order, default=-7.5),
              B.resample(src, *geom, order=order, default=-7.5), "order %d" % order)


@pytest.mark.parametrize("order", ORDERS)
def test_downsampling_and_a_two_plane_source(ctx, order):
    """three to one: neighbouring output planes share few source planes or none; and a source of
    two planes, where the mirror folds every tap onto the same two"""
    src = _source((40, 41, 42), np.int16, seed=12)
    geom = ((0.7, 0.7, 2.5), (1, 2, 3), (13, 14, 15), (2.1, 2.1, 7.5), (1.7, 2.7, 5.5))
    for extrapolate in (False, True):
        _same(ctx.resample_bspline(src, *geom, order=order, extrapolate=extrapolate, default=-7.5),
              B.resample(src, *geom, order=order, extrapolate=extrapolate, default=-7.5), "order %d" % order)
    src = _source((2, 9, 11), seed=13)
    geom = ((0.7, 0.7, 2.5), (0, 0, 0), (19, 13, 16), (0.5, 0.5, 0.25), (-0.2, 0.1, -1.4))
    _same(ctx.resample_bspline(src, *geom, order=order, extrapolate=True),
          B.resample(src, *geom, order=order, extrapolate=True), "two planes, order %d" % order)


def test_device_pointers_twice_back_to_back(ife):
    import torch
    src = _source(G_SRC["shape"], np.float32, seed=11)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with ife.Context(0) as c:
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_src = torch.from_numpy(src).to(dev)
            d_out = torch.full(G_DST["shape"], float("nan"), dtype=torch.float32, device=dev)
            d_src64 = d_src.double()
            d_out64 = torch.full(G_DST["shape"], float("nan"), dtype=torch.float64, device=dev)
            stream.synchronize()
            # the second call rewrites the host tables and the workspace behind the first
            c.resample_bspline_device(d_src.data_ptr(), ife.F32, src.shape, *G_GEOM, d_out.data_ptr(),
                                      translation=G_T, order=5, default=-7.5)
            c.resample_bspline_device(d_src64.data_ptr(), None, src.shape, *G_GEOM, d_out64.data_ptr(),
                                      translation=(0, 0, 0), order=2, extrapolate=True, default=-7.5)
            stream.synchronize()
            got, got64 = d_out.cpu().numpy(), d_out64.cpu().numpy()
    _same(got, B.resample(src, *G_GEOM, G_T, 5, False, -7.5), "first call")
    _same(got64, B.resample(src.astype(np.float64), *G_GEOM, (0, 0, 0), 2, True, -7.5), "second call")


# ---- window -------------------------------------------------------------------------------------

def _window_values(n, lo, hi, seed):
    edge = [lo, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), hi, np.nextafter(hi, -np.inf),
            np.nextafter(hi, np.inf), np.nan, np.inf, -np.inf, 0.0, -0.0]
    v = np.random.default_rng(seed).uniform(lo - 300.0, hi + 300.0, n)
    v[:min(n, len(edge))] = edge[:n]
    return v


@pytest.mark.parametrize("n", [1, 11, 256, 1000, LINE_CAP + 3], ids=["one", "edges", "a_block", "ragged", "beyond_cap"])
def test_window(ctx, n):
    lo, hi = -1250.0, 250.0                                   # level -500, width 1500
    v = _window_values(n, lo, hi, n)
    mask = (np.random.default_rng(n + 1).integers(0, 3, n) * 0.5).astype(np.float64)
    for kw in (dict(), dict(mask=mask), dict(mask=mask, out_min=3, out_max=200), dict(out_min=200, out_max=3)):
        got = ctx.window_u8(v, lo, hi, **kw)
        assert got.dtype == np.uint8 and np.array_equal(got, B.window_u8(v, lo, hi, **kw)), kw
    if n >= 11:
        first = ctx.window_u8(v, lo, hi)[:9].tolist()         # the ends themselves may round either way
        assert first[:3] == [0, 0, 0] and first[3] in (254, 255) and first[4] in (254, 255)
        assert first[5:] == [255, 0, 255, 0]                  # above, NaN, +inf, -inf
        got = ctx.window_u8(v, lo, hi, mask=mask, out_min=3)
        assert (got[mask == 0] == 0).all() and (got[mask != 0] >= 3).all()


# ---- arguments ----------------------------------------------------------------------------------

def test_argument_errors(ife, ctx):
    import torch
    dev = torch.device("cuda", 0)
    shape, dshape = (4, 5, 6), (5, 6, 7)
    d_src = torch.ones(4 * 5 * 6 + 1, dtype=torch.float64, device=dev)     # room for either source type
    d_out = torch.zeros(5 * 6 * 7 + 1, dtype=torch.float64, device=dev)    # room for every output
    torch.cuda.synchronize()
    sp, o = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    sptr, optr = d_src.data_ptr(), d_out.data_ptr()
    nan, inf = float("nan"), float("inf")

    def refused(code, src=sptr, dtype=ife.F32, sshape=shape, ssp=sp, so=o, dsh=dshape, dsp=sp, do=o, out=optr,
                tr=o, order=3, extrapolate=0, default=0.0):
        with pytest.raises(ife.IfeError) as e:
            ctx.resample_bspline_device(src, dtype, sshape, ssp, so, dsh, dsp, do, out, translation=tr, order=order,
                                        extrapolate=extrapolate, default=default)
        assert e.value.code == code, e.value

    for dtype in (ife.F32, None):
        refused(ife.E_ARG, dtype=dtype, order=-1)                  # the order and the extrapolation
        refused(ife.E_ARG, dtype=dtype, order=6)
        refused(ife.E_ARG, dtype=dtype, extrapolate=2)
        refused(ife.E_ARG, dtype=dtype, extrapolate=-1)
        refused(ife.E_ARG, dtype=dtype, src=0)                     # and everything ife_resample refuses
        refused(ife.E_ARG, dtype=dtype, out=0)
        refused(ife.E_ARG, dtype=dtype, so=(0, nan, 0))
        refused(ife.E_ARG, dtype=dtype, do=(inf, 0, 0))
        refused(ife.E_ARG, dtype=dtype, tr=(0, 0, -inf))
        refused(ife.E_ARG, dtype=dtype, default=nan)
        refused(ife.E_ARG, dtype=dtype, default=inf)
        refused(ife.E_ARG, dtype=dtype, out=optr + 4 if dtype is None else optr + 2)   # misaligned
        refused(ife.E_ARG, dtype=dtype, src=sptr + 2)
        refused(ife.E_SIZE, dtype=dtype, sshape=(4, 0, 6))
        refused(ife.E_SIZE, dtype=dtype, dsh=(5, 6, -1))
        refused(ife.E_ARG, dtype=dtype, ssp=(1, 0, 1))
        refused(ife.E_ARG, dtype=dtype, dsp=(1, 1, nan))
        refused(ife.E_ARG, dtype=dtype, out=sptr + 8, dsh=(1, 1, 2))   # output inside the source
        refused(ife.E_ARG, dtype=dtype, src=optr + 8, sshape=(1, 1, 2))
    refused(ife.E_ARG, dtype=7)                                    # unknown dtype
    refused(ife.E_ARG, dtype=-1)
    refused(ife.E_ARG, default=0.1)                                # not a float
    refused(ife.E_ARG, default=1e39)
    lib, d = ife.load_library(), ife.VolumeDesc(6, 5, 4, 1.0, 1.0, 1.0)
    z3 = (C.c_double * 3)(0, 0, 0)
    for args in ((None, C.byref(d), z3, z3), (z3, None, z3, z3), (z3, C.byref(d), None, z3),
                 (z3, C.byref(d), z3, None)):
        rc = lib.ife_resample_bspline(ctx._h, C.c_void_p(sptr), ife.F32, C.byref(d), args[0], args[1], args[2],
                                      args[3], 3, 0, 0.0, C.c_void_p(optr), ife.MEM_DEVICE)
        assert rc == ife.E_ARG

    def coef_refused(code, src=sptr, dtype=None, sshape=shape, order=3, coef=optr):
        with pytest.raises(ife.IfeError) as e:
            ctx.bspline_coefficients_device(src, dtype, sshape, order, coef)
        assert e.value.code == code, e.value

    for dtype in (ife.F32, None):
        coef_refused(ife.E_ARG, dtype=dtype, order=-1)
        coef_refused(ife.E_ARG, dtype=dtype, order=6)
        coef_refused(ife.E_ARG, dtype=dtype, src=0)
        coef_refused(ife.E_ARG, dtype=dtype, coef=0)
        coef_refused(ife.E_ARG, dtype=dtype, coef=optr + 4)        # misaligned
        coef_refused(ife.E_SIZE, dtype=dtype, sshape=(4, 0, 6))
        coef_refused(ife.E_ARG, dtype=dtype, src=optr + 8, sshape=(1, 1, 4))   # overlap that is not "in place"
    coef_refused(ife.E_ARG, dtype=ife.F32, src=optr)               # in place is for doubles only
    coef_refused(ife.E_ARG, dtype=7)

    d_u8 = torch.zeros(64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def window_refused(code, src=sptr, mask=0, n=16, lo=0.0, hi=1.0, out=d_u8.data_ptr()):
        with pytest.raises(ife.IfeError) as e:
            ctx.window_u8_device(src, mask, n, lo, hi, out)
        assert e.value.code == code, e.value

    window_refused(ife.E_ARG, lo=1.0, hi=1.0)                      # window_max <= window_min
    window_refused(ife.E_ARG, lo=2.0, hi=1.0)
    window_refused(ife.E_ARG, lo=nan)
    window_refused(ife.E_ARG, hi=inf)
    window_refused(ife.E_ARG, lo=-inf)
    window_refused(ife.E_SIZE, n=0)
    window_refused(ife.E_SIZE, n=-3)
    window_refused(ife.E_ARG, src=0)
    window_refused(ife.E_ARG, out=0)
    window_refused(ife.E_ARG, src=sptr + 4)
    window_refused(ife.E_ARG, out=sptr + 8)                        # output inside the source
    with pytest.raises(TypeError):
        ctx.resample_bspline(np.zeros(shape, np.int32), sp, o, dshape, sp, o)
    with pytest.raises(TypeError):
        ctx.bspline_coefficients(np.zeros(shape, np.int32))
    ctx.synchronize()
    # nothing was written by the refused calls
    assert (d_out == 0).all() and (d_src == 1).all() and (d_u8 == 0).all()
    # and ife_resample still refuses interpolation 2
    with pytest.raises(ife.IfeError):
        ctx.resample(np.zeros(shape, np.float32), sp, o, dshape, sp, o, interpolation=2)
