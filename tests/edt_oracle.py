"""numpy oracle of the signed distance map (ife_signed_distance_map), independent of the
algorithm under test: brute-force min-plus, no envelopes, no ballots.

  fg        mask != 0
  contour   fg voxels with a background face neighbour INSIDE the volume
  D2(v)     min over contour voxels c of ((hx(c)-hx(v))^2 + (hy(c)-hy(v))^2) + (hz(c)-hz(v))^2,
            h(i) = float64(i) * spacing, every operation rounded on its own; DBL_MAX where the
            volume has no contour voxel

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


def sq_dist(site, spacing=(1.0, 1.0, 1.0)):
    """Separable form: x, then y, then z, the order in which D2 accumulates its terms."""
    site = np.asarray(site, bool)
    hx, hy, hz = _coords(site.shape, spacing)
    g = np.where(site, 0.0, DBL_MAX)
    g = _minplus(g, hx, 2)
    g = _minplus(g, hy, 1)
    return _minplus(g, hz, 0)


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


def signed_distance_map(mask, spacing=(1.0, 1.0, 1.0), inside_is_positive=True, squared=False):
    fg = np.asarray(mask) != 0
    d2 = sq_dist(contour(fg), spacing)
    val = d2 if squared else np.sqrt(d2)
    return np.where(fg == bool(inside_is_positive), val, -val)


def expected_distance_terms(mask, prob, spacing=(1.0, 1.0, 1.0)):
    """The terms out(v) * prob(v) of the foreground voxels, in raster order."""
    fg = np.asarray(mask) != 0
    return (signed_distance_map(mask, spacing)[fg] * np.asarray(prob, np.float64)[fg])
