"""ife_resample / ife_resample_f64 on the device against the numpy oracle (tests/resample_oracle.py),
bit for bit in every case: the axis tables are the same IEEE operations on host and in numpy, and
the nested lerps round separately on the device (-ffp-contract=off) as numpy's do.  Floats are
compared as integers so that NaNs count.

The launch caps its grid at 2^20 workgroups (one per output row) and loops over the rows beyond:
test_rows_beyond_the_grid_cap takes the second trip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_oracle as R  # noqa: E402

pytestmark = pytest.mark.gpu

# the general geometry: part of every axis of the output lies outside the source
G_SRC = dict(shape=(5, 9, 70), spacing=(0.7, 0.7, 2.5), origin=(-100.3, 5.0, -7.0))
G_DST = dict(shape=(21, 13, 67), spacing=(0.9, 0.55, 0.625), origin=(-98.1, 4.1, -8.0))
G_T = (0.4, 0.0, 0.2)
DTYPES = {"f32": np.float32, "i16": np.int16, "u8": np.uint8, "u16": np.uint16, "f64": np.float64}


def _source(shape, dtype, seed=1):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype == np.uint16:
        return np.asarray([0, 1, 2, 300], np.uint16)[rng.integers(0, 4, shape)]
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)
    return (rng.standard_normal(shape) * 1000).astype(dtype)


def _check(ctx, src, s_spacing, s_origin, d_shape, d_spacing, d_origin, translation=(0, 0, 0), default=0.0,
           interps=(R.LINEAR, R.NEAREST)):
    """device == oracle bit for bit; returns the linear (or only) result"""
    first = None
    for interp in interps:
        want = R.resample(src, s_spacing, s_origin, d_shape, d_spacing, d_origin, translation, interp, default)
        got = ctx.resample(src, s_spacing, s_origin, d_shape, d_spacing, d_origin, translation, interp, default)
        assert got.dtype == want.dtype and got.shape == want.shape
        bad = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
        assert bad.size == 0, "interp %d: %d voxels differ, first %d: %r != %r" % (
            interp, bad.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])
        first = got if first is None else first
    return first


def test_general_geometry_inside_fraction():
    """what the case is chosen for: 52/67, 11/13 and 20/21 of the output inside, 62.5 % in all"""
    tx, ty, tz = R.tables(G_SRC["shape"], G_SRC["spacing"], G_SRC["origin"], G_DST["shape"], G_DST["spacing"],
                          G_DST["origin"], G_T)
    assert (int(tx[0].sum()), int(ty[0].sum()), int(tz[0].sum())) == (52, 11, 20)
    assert not tx[0][-1] and not ty[0][0] and not tz[0][-1]      # the low end of y, the high end of x and z


@pytest.mark.parametrize("interp", [R.LINEAR, R.NEAREST], ids=["linear", "nearest"])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_general_geometry_every_type(ctx, name, interp):
    src = _source(G_SRC["shape"], DTYPES[name])
    default = -7.5 if (interp == R.LINEAR or name in ("f32", "f64")) else (-7 if name == "i16" else 7)
    got = _check(ctx, src, G_SRC["spacing"], G_SRC["origin"], G_DST["shape"], G_DST["spacing"], G_DST["origin"],
                 G_T, default, interps=(interp,))
    want_dtype = (np.float64 if name == "f64" else np.float32) if interp == R.LINEAR else DTYPES[name]
    assert got.dtype == want_dtype
    assert abs((got == default).mean() - 0.375) < 0.01           # a forgotten default cannot pass on zeros
    if name == "u16" and interp == R.NEAREST:
        assert set(np.unique(got)) == {0, 1, 2, 7, 300}          # labels stay labels


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_dyadic_identity_returns_the_source(ctx, dtype):
    src = _source((6, 9, 70), dtype, 2)
    src[0, 0, 0], src[5, 8, 69], src[2, 3, 4], src[3, 3, 33] = np.inf, -np.inf, np.nan, np.inf
    src[1, 1, 1] = -np.nan
    sp, o = (0.75, 0.75, 0.75), (-3.25, -3.25, -3.25)
    for interp in (R.LINEAR, R.NEAREST):
        got = ctx.resample(src, sp, o, src.shape, sp, o, interpolation=interp, default=-7.5)
        assert np.array_equal(R.bits(got), R.bits(src))          # the select in L, not 0 * inf
    _check(ctx, src, sp, o, src.shape, sp, o, default=-7.5)


def test_non_dyadic_identity_equals_the_oracle(ctx):
    src = _source((6, 9, 70), np.float64, 3)
    sp, o = (0.7, 0.7, 0.7), (-3.3, 0.1, 12.7)
    _check(ctx, src, sp, o, src.shape, sp, o, default=-7.5)


@pytest.mark.parametrize("shape", [(1, 1, 200), (5, 1, 1), (1, 64, 65)], ids=["only_x", "only_z", "one_plane"])
def test_axes_of_length_one(ctx, shape):
    sp, o = (0.7, 0.9, 2.5), (1.0, -2.0, 3.0)
    dst = tuple(2 * n for n in shape)
    for dtype in (np.float64, np.int16):
        _check(ctx, _source(shape, dtype, 4), sp, o, dst, tuple(s / 2 for s in sp), o, default=-7)


@pytest.mark.parametrize("nx", [3, 63, 65, 300, 1027])
def test_rows_wider_than_a_workgroup_and_off_the_wave_width(ctx, nx):
    src = _source((3, 4, 130), np.float32, 5)
    s_t = 0.7 * 131.0 / nx          # a little more than the source's extent: outside at the far end
    _check(ctx, src, (0.7, 0.7, 2.5), (0, 0, 0), (4, 5, nx), (s_t, 0.6, 2.0), (-0.2, 0.1, 0.3), default=-7.5)


def test_downsampling_three_to_one(ctx):
    src = _source((70, 70, 70), np.int16, 6)
    _check(ctx, src, (0.7, 0.7, 2.5), (1, 2, 3), (23, 23, 23), (2.1, 2.1, 7.5), (1, 2, 3), default=-7)
    _check(ctx, src, (0.7, 0.7, 2.5), (1, 2, 3), (23, 23, 23), (2.1, 2.1, 7.5), (1.7, 2.7, 5.5), default=-7)


@pytest.mark.parametrize("translation", [(1e300, 0, 0), (0, 0, -1e300)])
def test_all_outside(ctx, translation):
    src = _source(G_SRC["shape"], np.float32)
    got = _check(ctx, src, G_SRC["spacing"], G_SRC["origin"], G_DST["shape"], G_DST["spacing"], G_DST["origin"],
                 translation, default=-7.5)
    assert (got == -7.5).all()


def test_the_tools_convention(ctx):
    """T = O_s - O_t: the origins cancel and the two index-zero voxels are aligned"""
    o_s, o_t = (-120.5, 37.25, 0.0), (37.25, -120.5, 8.0)
    t = tuple(a - b for a, b in zip(o_s, o_t))
    src = _source((6, 10, 12), np.float64, 7)
    got = _check(ctx, src, (0.75, 0.75, 2.5), o_s, (24, 10, 12), (0.75, 0.75, 0.625), o_t, t, default=-7.5)
    assert np.array_equal(got[::4][:6], src)              # every fourth plane is a source plane
    assert (got[21] == src[5]).all() and (got[22:] == -7.5).all()      # c = 5.25: edge extended; 5.5: outside


def test_rows_beyond_the_grid_cap(ctx):
    """1025 * 1024 rows of three voxels: the workgroups of the capped grid take a second row"""
    src = _source((9, 8, 3), np.float64, 8)
    d_shape = (1025, 1024, 3)
    assert d_shape[0] * d_shape[1] > 1 << 20
    _check(ctx, src, (1.0, 1.0, 1.0), (0, 0, 0), d_shape, (0.9, 8.0 / 1024, 9.5 / 1025), (-0.3, -0.2, -0.4),
           default=-7.5, interps=(R.LINEAR,))


def test_device_pointers_on_a_side_stream(ife):
    import torch
    src = _source(G_SRC["shape"], np.float32)
    geom = (G_SRC["spacing"], G_SRC["origin"], G_DST["shape"], G_DST["spacing"], G_DST["origin"])
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
            # two calls back to back: the second rewrites the host tables behind the first's upload
            c.resample_device(d_src.data_ptr(), ife.F32, src.shape, *geom, d_out.data_ptr(), translation=G_T,
                              default=-7.5)
            c.resample_device(d_src64.data_ptr(), None, src.shape, *geom, d_out64.data_ptr(),
                              translation=(0, 0, 0), interpolation=ife.INTERP_NEAREST, default=-7.5)
            stream.synchronize()
            got, got64 = d_out.cpu().numpy(), d_out64.cpu().numpy()
        want = R.resample(src, *geom, G_T, R.LINEAR, -7.5)
        assert np.array_equal(R.bits(got), R.bits(want))
        want64 = R.resample(src.astype(np.float64), *geom, (0, 0, 0), R.NEAREST, -7.5)
        assert np.array_equal(R.bits(got64), R.bits(want64))


def test_argument_errors(ife, ctx):
    import torch
    dev = torch.device("cuda", 0)
    shape, dshape = (4, 5, 6), (5, 6, 7)
    d_src = torch.ones(4 * 5 * 6 + 1, dtype=torch.float32, device=dev)
    d_out = torch.zeros(5 * 6 * 7 + 1, dtype=torch.float64, device=dev)    # room for either call
    torch.cuda.synchronize()
    sp, o = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    sptr, optr = d_src.data_ptr(), d_out.data_ptr()
    nan, inf = float("nan"), float("inf")

    def refused(code, src=sptr, dtype=ife.F32, sshape=shape, ssp=sp, so=o, dsh=dshape, dsp=sp, do=o, out=optr,
                tr=o, interp=ife.INTERP_LINEAR, default=0.0):
        with pytest.raises(ife.IfeError) as e:
            ctx.resample_device(src, dtype, sshape, ssp, so, dsh, dsp, do, out, translation=tr,
                                interpolation=interp, default=default)
        assert e.value.code == code, e.value

    for dtype in (ife.F32, None):
        refused(ife.E_ARG, dtype=dtype, src=0)                     # null pointers
        refused(ife.E_ARG, dtype=dtype, out=0)
        refused(ife.E_ARG, dtype=dtype, interp=2)                  # unknown interpolation
        refused(ife.E_ARG, dtype=dtype, so=(0, nan, 0))            # non-finite geometry and default
        refused(ife.E_ARG, dtype=dtype, do=(inf, 0, 0))
        refused(ife.E_ARG, dtype=dtype, tr=(0, 0, -inf))
        refused(ife.E_ARG, dtype=dtype, default=nan)
        refused(ife.E_ARG, dtype=dtype, default=inf)
        refused(ife.E_ARG, dtype=dtype, out=optr + 4 if dtype is None else optr + 2)   # misaligned
        refused(ife.E_ARG, dtype=dtype, src=sptr + 2)
        refused(ife.E_SIZE, dtype=dtype, sshape=(4, 0, 6))         # non-positive sizes
        refused(ife.E_SIZE, dtype=dtype, dsh=(5, 6, -1))
        refused(ife.E_ARG, dtype=dtype, ssp=(1, 0, 1))             # spacing as check_vol has it
        refused(ife.E_ARG, dtype=dtype, dsp=(1, 1, nan))
        refused(ife.E_ARG, dtype=dtype, out=sptr + 8, dsh=(1, 1, 2))   # output inside the source
        refused(ife.E_ARG, dtype=dtype, src=optr + 8, sshape=(1, 1, 2))
    refused(ife.E_ARG, dtype=7)                                    # unknown dtype
    refused(ife.E_ARG, dtype=-1)
    refused(ife.E_ARG, default=0.1)                                # not a float
    refused(ife.E_ARG, default=1e39)
    refused(ife.E_ARG, dtype=ife.U8, interp=ife.INTERP_NEAREST, default=0.5)
    refused(ife.E_ARG, dtype=ife.U8, interp=ife.INTERP_NEAREST, default=256)
    refused(ife.E_ARG, dtype=ife.U16, interp=ife.INTERP_NEAREST, default=-1)
    refused(ife.E_ARG, dtype=ife.I16, interp=ife.INTERP_NEAREST, default=32768)
    # null origins and descriptors: the C call itself
    lib, d = ife.load_library(), ife.VolumeDesc(6, 5, 4, 1.0, 1.0, 1.0)
    z3 = (C.c_double * 3)(0, 0, 0)
    for args in ((None, C.byref(d), z3, z3), (z3, None, z3, z3), (z3, C.byref(d), None, z3),
                 (z3, C.byref(d), z3, None)):
        rc = lib.ife_resample(ctx._h, C.c_void_p(sptr), ife.F32, C.byref(d), args[0], args[1], args[2], args[3],
                              0, 0.0, C.c_void_p(optr), ife.MEM_DEVICE)
        assert rc == ife.E_ARG
    with pytest.raises(TypeError):
        ctx.resample(np.zeros(shape, np.int32), sp, o, dshape, sp, o)
    ctx.synchronize()
    assert (d_out == 0).all() and (d_src == 1).all()               # nothing was written by the refused calls
    # and a default that IS a value of the type is taken
    got = ctx.resample(np.ones(shape, np.uint8), sp, o, dshape, sp, o, interpolation=ife.INTERP_NEAREST, default=255)
    assert got[4, 5, 6] == 255 and got[0, 0, 0] == 1
