"""The definition of the B-spline calls (include/ife_hip.h, DESIGN.md "B-spline resampling") in
numpy: poles, horizons, the recursive prefilter, the axis tables of the gather, the nested sums and
the 8-bit window.  Arrays are (nz, ny, nx); spacings, origins and the translation are (x, y, z)
triples.  float64 throughout, one operation per numpy call so that each rounds on its own.  The
checker of the plan program and of the device path, never the thing under test."""
import math

import numpy as np

F = np.float64
FLT_MAX = float(np.finfo(np.float32).max)
HORIZONS = {2: (14,), 3: (18,), 4: (23, 6), 5: (28, 8)}


def poles(order):
    s = math.sqrt                       # correctly rounded, as std::sqrt
    if order == 2:
        return (s(8.0) - 3.0,)
    if order == 3:
        return (s(3.0) - 2.0,)
    if order == 4:
        return (s(664.0 - s(438976.0)) + s(304.0) - 19.0, s(664.0 + s(438976.0)) - s(304.0) - 19.0)
    if order == 5:
        return (s(135.0 / 2.0 - s(17745.0 / 4.0)) + s(105.0 / 4.0) - 13.0 / 2.0,
                s(135.0 / 2.0 + s(17745.0 / 4.0)) - s(105.0 / 4.0) - 13.0 / 2.0)
    return ()


def gain(order):
    g = 1.0
    for z in poles(order):
        g = g * (1.0 - z) * (1.0 - 1.0 / z)
    return g


def start_table(z, h, n):
    """(full, first, multipliers of c[1 ..], divisor) of the causal start of a line of length n"""
    zn = z
    if h < n:
        m = []
        for _ in range(1, h):
            m.append(zn)
            zn = zn * z
        return False, 0.0, m, 1.0
    iz = 1.0 / z
    z2n = z
    for _ in range(n - 2):
        z2n = z2n * z
    first = z2n
    z2n = z2n * (z2n * iz)
    m = []
    for _ in range(1, n - 1):
        m.append(zn + z2n)
        zn = zn * z
        z2n = z2n * iz
    return True, first, m, 1.0 - zn * zn


def filter_lines(c, order):
    """the prefilter along axis 0 of c (float64, any further axes: the lines), in place"""
    n = c.shape[0]
    zs = poles(order)
    if n == 1 or not zs:
        return c
    c *= F(gain(order))
    for z, h in zip(zs, HORIZONS[order]):
        full, first, m, div = start_table(z, h, n)
        s = c[0].copy()
        if full:
            s = s + F(first) * c[n - 1]
        for k, mk in enumerate(m, 1):
            s = s + F(mk) * c[k]
        c[0] = s / F(div) if full else s
        for j in range(1, n):
            c[j] = c[j] + F(z) * c[j - 1]
        c[n - 1] = F(z / (z * z - 1.0)) * (F(z) * c[n - 2] + c[n - 1])
        for j in range(n - 2, -1, -1):
            c[j] = F(z) * (c[j + 1] - c[j])
    return c


def coefficients(src, order):
    """x, then y, then z; src of any of the library's dtypes, float64 out"""
    c = np.array(src, dtype=F, order="C")
    if order >= 2:
        for axis in (2, 1, 0):
            filter_lines(np.moveaxis(c, axis, 0), order)
    return c


def weights(order, w):
    """ITK's closed forms; w an array, the result has shape (order + 1,) + w.shape"""
    w = np.asarray(w, F)
    if order == 0:
        return np.ones((1,) + w.shape)
    if order == 1:
        return np.stack([1.0 - w, w])
    if order == 2:
        w1 = 0.75 - w * w
        w2 = 0.5 * (w - w1 + 1.0)
        return np.stack([1.0 - w1 - w2, w1, w2])
    if order == 3:
        w3 = (1.0 / 6.0) * w * w * w
        w0 = 1.0 / 6.0 + 0.5 * w * (w - 1.0) - w3
        w2 = w + w0 - 2.0 * w3
        return np.stack([w0, 1.0 - w0 - w2 - w3, w2, w3])
    if order == 4:
        w2_ = w * w
        t = (1.0 / 6.0) * w2_
        w0 = 0.5 - w
        w0 = w0 * w0
        w0 = w0 * ((1.0 / 24.0) * w0)
        t0 = w * (t - 11.0 / 24.0)
        t1 = 19.0 / 96.0 + w2_ * (0.25 - t)
        w1, w3 = t1 + t0, t1 - t0
        w4 = w0 + t0 + 0.5 * w
        return np.stack([w0, w1, 1.0 - w0 - w1 - w3 - w4, w3, w4])
    if order == 5:
        w2_ = w * w
        w5 = (1.0 / 120.0) * w * w2_ * w2_
        w2_ = w2_ - w
        w4_ = w2_ * w2_
        w = w - 0.5
        t = w2_ * (w2_ - 3.0)
        w0 = (1.0 / 24.0) * (1.0 / 5.0 + w2_ + w4_) - w5
        t0 = (1.0 / 24.0) * (w2_ * (w2_ - 5.0) + 46.0 / 5.0)
        t1 = (-1.0 / 12.0) * w * (t + 4.0)
        w2, w3 = t0 + t1, t0 - t1
        t0 = (1.0 / 16.0) * (9.0 / 5.0 - t)
        t1 = (1.0 / 24.0) * w * (w4_ - w2_ - 5.0)
        return np.stack([w0, t0 + t1, w2, w3, t0 - t1, w5])
    raise ValueError("order %r" % (order,))


def mirror(i, n):
    P = 2 * n - 2
    i = np.abs(i) % P
    return np.where(i >= n, P - i, i)


def axis_table(order, n_t, n_s, s_s, o_s, s_t, o_t, tr):
    """inside (n_t bools), e (n_t), idx (n_t, K), w (n_t, K); idx and w are 0 where outside and
    beyond the single tap of a source axis of length 1"""
    K = order + 1
    with np.errstate(over="ignore", invalid="ignore"):
        p = F(o_t) + np.arange(n_t, dtype=F) * F(s_t)
        q = p + F(tr)
        c = (q - F(o_s)) / F(s_s)
        inside = (c >= -0.5) & (c < F(n_s - 1) + 0.5)
        hi, mid = c >= F(n_s - 1), c > 0.0
    cm = np.where(mid & ~hi, c, 0.0)
    e = np.where(hi, n_s - 1, np.where(mid, np.minimum(np.floor(cm + 0.5).astype(np.int64), n_s - 1), 0))
    idx, w = np.zeros((n_t, K), np.int64), np.zeros((n_t, K))
    if n_s == 1:
        w[inside, 0] = 1.0
        return inside, e, idx, w
    ci = np.where(inside, c, 0.0)
    i0 = np.floor(ci if order & 1 else ci + 0.5).astype(np.int64) - order // 2
    wt = weights(order, ci - (i0 + order // 2).astype(F)).T
    taps = mirror(i0[:, None] + np.arange(K)[None, :], n_s)
    idx[inside], w[inside] = taps[inside], wt[inside]
    return inside, e, idx, w


def tables(order, src_shape, src_spacing, src_origin, dst_shape, dst_spacing, dst_origin, translation):
    """The x, y and z tables."""
    return [axis_table(order, dst_shape[2 - d], src_shape[2 - d], src_spacing[d], src_origin[d], dst_spacing[d],
                       dst_origin[d], translation[d]) for d in range(3)]


def resample(src, src_spacing, src_origin, dst_shape, dst_spacing, dst_origin, translation=(0, 0, 0), order=3,
             extrapolate=False, default=0.0):
    """float64 in: float64 out; any other dtype: float32 (one rounding, clamped to +-FLT_MAX)"""
    src = np.asarray(src)
    odt = np.float64 if src.dtype == np.float64 else np.float32
    coef = coefficients(src, order)
    tx, ty, tz = tables(order, src.shape, src_spacing, src_origin, dst_shape, dst_spacing, dst_origin, translation)
    kx, ky, kz = (1 if n == 1 else order + 1 for n in (src.shape[2], src.shape[1], src.shape[0]))
    v = None
    for k in range(kz):
        s = None
        for j in range(ky):
            rows = coef[tz[2][:, k][:, None], ty[2][:, j][None, :]]      # (nz_t, ny_t, nx_s)
            r = None
            for i in range(kx):
                prod = tx[3][:, i][None, None, :] * rows[:, :, tx[2][:, i]]
                r = prod if r is None else r + prod
            prod = ty[3][:, j][None, :, None] * r
            s = prod if s is None else s + prod
        prod = tz[3][:, k][:, None, None] * s
        v = prod if v is None else v + prod
    if odt == np.float32:
        v = np.where(v > FLT_MAX, FLT_MAX, np.where(v < -FLT_MAX, -FLT_MAX, v)).astype(np.float32)
    inside = tz[0][:, None, None] & ty[0][None, :, None] & tx[0][None, None, :]
    if extrapolate:
        outside = src[tz[1][:, None, None], ty[1][None, :, None], tx[1][None, None, :]].astype(odt)
    else:
        outside = odt(default)
    return np.where(inside, v, outside).astype(odt)


def window_u8(src, window_min, window_max, mask=None, out_min=0, out_max=255):
    v = np.asarray(src, F)
    scale = (F(out_max) - F(out_min)) / (F(window_max) - F(window_min))
    shift = F(out_min) - F(window_min) * scale
    with np.errstate(invalid="ignore", over="ignore"):
        y = v * scale + shift
        lin = np.where(y > 0.0, np.where(y > 255.0, 255.0, y), 0.0)
        mid = (v >= window_min) & (v <= window_max)
        r = np.where(v > window_max, out_max, np.where(mid, np.where(mid, lin, 0.0).astype(np.int64), out_min))
    r = r.astype(np.uint8)
    if mask is not None:
        r = np.where(np.asarray(mask, F) != 0, r, 0).astype(np.uint8)
    return r


def bits(a):
    """The array as unsigned integers of its element size, so that NaNs compare."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
