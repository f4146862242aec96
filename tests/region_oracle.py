"""numpy restatements of the region calls (include/ife_hip.h, DESIGN.md "Regions"): what the device
results and the host plan are held equal to.  Volumes are (z, y, x) arrays, boxes {x, y, z}."""
import numpy as np


def foreground(mask):
    """integers: != 0; float32: any bit pattern but +-0 (denormals and NaN are foreground)"""
    mask = np.asarray(mask)
    if mask.dtype == np.float32:
        return (np.ascontiguousarray(mask).view(np.uint32) & 0x7fffffff) != 0
    return mask != 0


def bounding_box(mask):
    """((x0, y0, z0), (sx, sy, sz), count); zeros for an empty mask"""
    idx = np.argwhere(foreground(mask))
    if idx.shape[0] == 0:
        return (0, 0, 0), (0, 0, 0), 0
    lo, hi = idx.min(axis=0), idx.max(axis=0)
    return (tuple(int(v) for v in lo[::-1]), tuple(int(v) for v in (hi - lo + 1)[::-1]), int(idx.shape[0]))


def extract_region(src, index_xyz, size_xyz, pad_value=None, flip=(False, False, False)):
    """np.full with the pad value, the overlap with the source sliced in, then np.flip"""
    src = np.asarray(src)
    index, size = [int(v) for v in index_xyz][::-1], [int(v) for v in size_xyz][::-1]   # z, y, x
    inside = all(i >= 0 and i + s <= n for i, s, n in zip(index, size, src.shape))
    if pad_value is None:
        assert inside, "a region that reaches outside needs a pad value"
        pad_value = 0
    out = np.full(size, pad_value, src.dtype)
    lo = [max(i, 0) for i in index]
    hi = [min(i + s, n) for i, s, n in zip(index, size, src.shape)]
    if all(h > l for l, h in zip(lo, hi)):
        dst = tuple(slice(l - i, h - i) for l, h, i in zip(lo, hi, index))
        out[dst] = src[tuple(slice(l, h) for l, h in zip(lo, hi))]
    axes = [2 - a for a in range(3) if flip[a]]   # flip is (x, y, z)
    return np.ascontiguousarray(np.flip(out, axes)) if axes else out


def axis_split(idx, size, n_src, flip):
    """(lo, n, hi, src0, step) of one output axis: output [lo, lo + n) is copied, output index
    lo + k from source index src0 + k * step; the rest is pad.  By enumeration."""
    srcs = [idx + (size - 1 - i if flip else i) for i in range(size)]
    inside = [i for i, s in enumerate(srcs) if 0 <= s < n_src]
    step = -1 if flip else 1
    if not inside:
        return size, 0, 0, 0, step
    lo, n = inside[0], len(inside)
    assert inside == list(range(lo, lo + n))
    return lo, n, size - lo - n, srcs[lo], step


def label_membership(labels, include, inside=1, outside=0):
    labels = np.asarray(labels)
    return np.where(np.isin(labels, np.asarray(list(include), np.int64)), inside, outside).astype(labels.dtype)


# ---- geometry of a cropped or padded output, in double ------------------------------------------
def shift_origin(origin, spacing, index):
    return np.asarray(origin, np.float64) + np.asarray(index, np.float64) * np.asarray(spacing, np.float64)


def shift_srow(srow, index):
    """srow (3, 4) float32 -> the fourth column in double: srow[r][3] + sum_a srow[r][a] * index[a]"""
    s = np.asarray(srow, np.float32).astype(np.float64)
    return s[:, 3] + s[:, :3] @ np.asarray(index, np.float64)


def quaternion_rotation(b, c, d):
    b, c, d = float(b), float(c), float(d)
    a = 1.0 - (b * b + c * c + d * d)
    if a < 1e-7:
        a = 1.0 / np.sqrt(b * b + c * c + d * d)
        b, c, d, a = b * a, c * a, d * a, 0.0
    else:
        a = np.sqrt(a)
    return np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                     [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                     [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]], np.float64)


def shift_qoffset(quatern, qfac, pixdim, qoffset, index):
    """the qoffset in double: qoffset + R(quatern) (qfac on the z column) (pixdim o index)"""
    q = [float(np.float32(v)) for v in quatern]
    v = np.asarray(pixdim, np.float64) * np.asarray(index, np.float64)
    v[2] *= -1.0 if float(qfac) < 0 else 1.0
    return np.asarray(qoffset, np.float32).astype(np.float64) + quaternion_rotation(*q) @ v


def within_one_ulp(got_f32, want_f64):
    """every float32 of got is one of the two float32 neighbours of the double (or equal)"""
    got = np.asarray(got_f32, np.float32)
    want = np.asarray(want_f64, np.float64)
    near = want.astype(np.float32)
    lo, hi = np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))
    return bool(np.all((got >= lo) & (got <= hi)))
