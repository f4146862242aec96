"""The definition of ife_resample (include/ife_hip.h, DESIGN.md "Resampling") in numpy: the axis
tables, then the nested selects.  Arrays are (nz, ny, nx); spacings, origins and the translation
are (x, y, z) triples.  float64 throughout, one operation per numpy call so that each rounds on
its own.  The checker of the plan program and of the device path, never the thing under test."""
import numpy as np

LINEAR, NEAREST = 0, 1


def axis_table(n_t, n_s, s_s, o_s, s_t, o_t, tr):
    """inside (bool), b, t, skip (bool), near per output index; b, t, skip and near are 0 / 0.0 /
    False where outside (nothing outside is converted to an integer)."""
    f = np.float64
    with np.errstate(over="ignore", invalid="ignore"):
        p = f(o_t) + np.arange(n_t, dtype=f) * f(s_t)
        q = p + f(tr)
        c = (q - f(o_s)) / f(s_s)
        inside = (c >= -0.5) & (c < f(n_s - 1) + 0.5)
    ci = np.where(inside, c, 0.0)
    b = np.maximum(np.floor(ci).astype(np.int64), 0)
    t = np.where(inside, ci - b.astype(f), 0.0)
    skip = inside & ((t <= 0) | (b + 1 > n_s - 1))
    near = np.minimum(np.floor(ci + 0.5).astype(np.int64), n_s - 1)
    return inside, np.where(inside, b, 0), t, skip, np.where(inside, near, 0)


def tables(src_shape, src_spacing, src_origin, dst_shape, dst_spacing, dst_origin, translation):
    """The x, y and z tables."""
    return [axis_table(dst_shape[2 - d], src_shape[2 - d], src_spacing[d], src_origin[d], dst_spacing[d],
                       dst_origin[d], translation[d]) for d in range(3)]


def _lerp(a, b, t, skip):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(skip, a, a + (b - a) * t)


def resample(src, src_spacing, src_origin, dst_shape, dst_spacing, dst_origin, translation=(0, 0, 0),
             interpolation=LINEAR, default=0.0):
    """float64 in: float64 out.  Any other dtype: float32 (linear, one rounding of the double
    value) or the source's dtype (nearest)."""
    src = np.asarray(src)
    tx, ty, tz = tables(src.shape, src_spacing, src_origin, dst_shape, dst_spacing, dst_origin, translation)
    inside = tz[0][:, None, None] & ty[0][None, :, None] & tx[0][None, None, :]
    if interpolation == NEAREST:
        val = src[tz[4][:, None, None], ty[4][None, :, None], tx[4][None, None, :]]
        return np.where(inside, val, np.asarray(default, src.dtype)).astype(src.dtype)
    odt = np.float64 if src.dtype == np.float64 else np.float32
    (bx, wx, kx), (by, wy, ky), (bz, wz, kz) = ((t[1], t[2], t[3]) for t in (tx, ty, tz))
    # a skipped axis never reads its upper neighbour: index b there (and outside, where b is 0)
    ux, uy, uz = (np.where(t[3] | ~t[0], t[1], t[1] + 1) for t in (tx, ty, tz))
    s = src.astype(np.float64)

    def v(z, y, x):
        return s[z[:, None, None], y[None, :, None], x[None, None, :]]

    WX, KX = wx[None, None, :], kx[None, None, :]
    WY, KY = wy[None, :, None], ky[None, :, None]
    WZ, KZ = wz[:, None, None], kz[:, None, None]
    vx00 = _lerp(v(bz, by, bx), v(bz, by, ux), WX, KX)
    vx10 = _lerp(v(bz, uy, bx), v(bz, uy, ux), WX, KX)
    vx01 = _lerp(v(uz, by, bx), v(uz, by, ux), WX, KX)
    vx11 = _lerp(v(uz, uy, bx), v(uz, uy, ux), WX, KX)
    vxy0 = _lerp(vx00, vx10, WY, KY)
    vxy1 = _lerp(vx01, vx11, WY, KY)
    val = _lerp(vxy0, vxy1, WZ, KZ)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(inside, val.astype(odt), odt(default))


def bits(a):
    """The array as unsigned integers of its element size, so that NaNs compare."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
