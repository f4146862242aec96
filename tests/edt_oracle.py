"""numpy oracle of the signed distance map (ife_signed_distance_map), independent of the
algorithm under test: brute-force min-plus, no envelopes, no ballots.

  fg        mask != 0
  contour   fg voxels with a background face neighbour INSIDE the volume
  D2(v)     min over contour voxels c of ((hx(c)-hx(v))^2 + (hy(c)-hy(v))^2) + (hz(c)-hz(v))^2,
            h(i) = float64(i) * spacing, every operation rounded on its own; DBL_MAX where the
            volume has no contour voxel

sq_dist(..., slabs=True) is the same arithmetic one slab at a time, for lines of a few hundred voxels;
expected_distance_device_order sums the terms of ife_expected_distance in the device's order.
ROW_PATTERNS / row_mask are the isolated-row masks that tests/test_gpu_distance.py runs and
tests/test_distance_cpu.py classifies.

Volumes are [z, y, x]; spacing is (sx, sy, sz)."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def contour(fg):
    """Six-neighbour contour by shifted comparisons; neighbours outside the volume do not count."""
    fg = np.asarray(fg, bool)
    bg_nb = np.zeros(fg.shape, bool)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        bg_nb[lo] |= ~fg[hi]   # the neighbour at +1
        bg_nb[hi] |= ~fg[lo]   # the neighbour at -1
    return fg & bg_nb


def _coords(shape, spacing):
    nz, ny, nx = shape
    sx, sy, sz = (np.float64(s) for s in spacing)
    return (np.arange(nx, dtype=np.float64) * sx, np.arange(ny, dtype=np.float64) * sy,
            np.arange(nz, dtype=np.float64) * sz)


def _minplus(g, h, axis):
    """out[i] = min over j of g[j] + (h[j] - h[i])^2 along `axis`: O(n^2) per line."""
    g = np.moveaxis(g, axis, -1)
    d = (h[:, None] - h[None, :]) ** 2                      # [j, i]
    out = np.min(g[..., :, None] + d, axis=-2)
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def _minplus_slabs(g, h, axis):
    """_minplus one slab of the leading axis at a time: the same sums and the same minimum, with an
    [n, n] temporary per line of one slab instead of the whole volume (lines of a few hundred)."""
    g = np.moveaxis(g, axis, -1)
    d = (h[:, None] - h[None, :]) ** 2                      # [j, i]
    out = np.empty(g.shape, np.float64)
    for k in range(g.shape[0]):
        out[k] = np.min(g[k][..., :, None] + d, axis=-2)
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def sq_dist(site, spacing=(1.0, 1.0, 1.0), slabs=False):
    """Separable form: x, then y, then z, the order in which D2 accumulates its terms.  `slabs`:
    slab by slab (_minplus_slabs), for volumes whose lines are too long for one temporary."""
    site = np.asarray(site, bool)
    hx, hy, hz = _coords(site.shape, spacing)
    minplus = _minplus_slabs if slabs else _minplus
    g = np.where(site, 0.0, DBL_MAX)
    g = minplus(g, hx, 2)
    g = minplus(g, hy, 1)
    return minplus(g, hz, 0)


def sq_dist_allpairs(site, spacing=(1.0, 1.0, 1.0)):
    """The definition itself, one site at a time (tiny volumes only)."""
    site = np.asarray(site, bool)
    hx, hy, hz = _coords(site.shape, spacing)
    out = np.full(site.shape, DBL_MAX)
    for z, y, x in zip(*np.nonzero(site)):
        d = ((hx[x] - hx)[None, None, :] ** 2 + (hy[y] - hy)[None, :, None] ** 2) \
            + (hz[z] - hz)[:, None, None] ** 2
        np.minimum(out, d, out=out)
    return out


def signed_distance_map(mask, spacing=(1.0, 1.0, 1.0), inside_is_positive=True, squared=False, slabs=False):
    fg = np.asarray(mask) != 0
    d2 = sq_dist(contour(fg), spacing, slabs)
    val = d2 if squared else np.sqrt(d2)
    return np.where(fg == bool(inside_is_positive), val, -val)


def expected_distance_terms(mask, prob, spacing=(1.0, 1.0, 1.0), slabs=False, dist=None):
    """The terms out(v) * prob(v) of the foreground voxels, in raster order.  `dist`: the map
    signed_distance_map(mask, spacing), where the caller has it already."""
    fg = np.asarray(mask) != 0
    if dist is None:
        dist = signed_distance_map(mask, spacing, slabs=slabs)
    return (dist[fg] * np.asarray(prob, np.float64)[fg])


# ---- isolated rows: masks whose foreground lies in one row, so that every other row leaves the x
# pass without a site and what the x pass writes in that row reaches every voxel ----------------
SEGMENT = 64           # voxels per ballot of edt_x_kernel (csrc/distance_kernels.hpp)

ROW_PATTERNS = {       # name: (nx, inclusive runs (first, last) of foreground along x)
    "300_at0": (300, [(0, 0)]),
    "300_at299": (300, [(299, 299)]),
    "300_at63": (300, [(63, 63)]),
    "300_at64": (300, [(64, 64)]),
    "300_at10_290": (300, [(10, 10), (290, 290)]),
    "300_run100_140": (300, [(100, 140)]),
    "320_at63_256": (320, [(63, 63), (256, 256)]),
    "320_at64_191": (320, [(64, 64), (191, 191)]),
    "320_run60_200": (320, [(60, 200)]),
    "65_at64": (65, [(64, 64)]),
}
ROW_ZY = (1, 2)        # the row of the foreground in the (3, 4, nx) form


def row_mask(name, volume, dtype=np.uint8, value=1):
    """(mask, (z, y) of its foreground row).  volume False: shape (1, 1, nx), where a run has sites
    at its two ends only; True: shape (3, 4, nx) with the foreground in row z = 1, y = 2, where
    every voxel of a run is a site."""
    nx, runs = ROW_PATTERNS[name]
    z, y = ROW_ZY if volume else (0, 0)
    mask = np.zeros((3, 4, nx) if volume else (1, 1, nx), dtype)
    for a, b in runs:
        mask[z, y, a:b + 1] = value
    return mask, (z, y)


def segment_occupancy(site_row):
    """Per 64-voxel segment of a row (the last one may be partial): does it hold a site?"""
    site_row = np.asarray(site_row, bool)
    pad = -site_row.size % SEGMENT
    return np.concatenate([site_row, np.zeros(pad, bool)]).reshape(-1, SEGMENT).any(axis=1)


REDUCE_THREADS = 256   # EDT_REDUCE_THREADS of csrc/distance_kernels.hpp


def expected_distance_device_order(mask, prob, spacing=(1.0, 1.0, 1.0), slabs=False, dist=None):
    """(mean, count) with the sum built in the order csrc/distance_kernels.hpp documents, every
    step an IEEE double operation: per z line the terms sqrt(D2) * prob of its foreground voxels in
    line order onto 0.0; thread t of 256 adds the sums of lines t, t + 256, ... in that order; the
    256 partial sums go through a binary tree (s[t] += s[t + o] for o = 128, 64, ... 1); sum / count.
    `dist` as in expected_distance_terms (only its foreground, where it is sqrt(D2), is read)."""
    fg = np.asarray(mask) != 0
    prob = np.asarray(prob, np.float64)
    if dist is None:
        dist = np.sqrt(sq_dist(contour(fg), spacing, slabs))
    nz = fg.shape[0]
    line = np.zeros(fg.shape[1:], np.float64)
    for z in range(nz):
        line = np.where(fg[z], line + dist[z] * prob[z], line)
    line = line.ravel()                                    # line number: x fastest, then y
    pad = -line.size % REDUCE_THREADS                      # s + 0.0 == s for the s >= +0.0 here
    rows = np.concatenate([line, np.zeros(pad)]).reshape(-1, REDUCE_THREADS)
    part = np.zeros(REDUCE_THREADS, np.float64)
    for r in rows:
        part = part + r
    o = REDUCE_THREADS // 2
    while o > 0:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    n = int(np.count_nonzero(fg))
    return (float(part[0] / np.float64(n)) if n else 0.0), n
