"""The rule of ife_roi_labels / ife_dense_roi_labels (include/ife_hip.h) in numpy.

For one box of a uint8 label volume, a set G of ignored labels and a dominant label d (-1: none):
n(l) = the number of voxels of the box that carry l, c(l) = 0 if l is in G, else n(l).

  1. d >= 0 and (n(d) > 0 or d in G): the label is d
  2. else max c > 0: the smallest l with c(l) = max c
  3. else: the smallest member of G

Where the maximum is unique this is tools/ExtractLabels.cxx:164-212; at ties the reference has no
defined answer (it takes whichever key its unordered_map iterates first), so "smallest" is ours.

Two independent forms: roi_labels / ties count box by box (a bincount per box), dense_labels /
dense_ties take the boxes of the dense generator all at once from 3-D cumulative sums.  They share
no code, and tests/test_labels_oracle_cpu.py holds them equal.
"""
import numpy as np


def box_label(counts, ignore=(), dominant=-1):
    """The label for the 256 counts n(l) of one box."""
    n = np.asarray(counts, np.int64)
    assert n.shape == (256,)
    G = sorted(set(int(v) for v in ignore))
    if dominant >= 0 and (n[dominant] > 0 or dominant in G):
        return int(dominant)
    c = n.copy()
    c[G] = 0
    if c.max() > 0:
        return int(np.argmax(c))          # argmax returns the first, that is the smallest, maximum
    return G[0]


def box_counts(labels, box):
    x, y, z, sx, sy, sz = (int(v) for v in box)
    nz, ny, nx = labels.shape
    assert sx >= 1 and sy >= 1 and sz >= 1 and x >= 0 and y >= 0 and z >= 0
    assert x + sx <= nx and y + sy <= ny and z + sz <= nz
    return np.bincount(labels[z:z + sz, y:y + sy, x:x + sx].ravel(), minlength=256)


def roi_labels(labels, rois, ignore=(), dominant=-1):
    """(n,) uint8: the label of every box {x, y, z, sx, sy, sz} of rois."""
    labels = np.asarray(labels)
    assert labels.dtype == np.uint8 and labels.ndim == 3
    rois = np.asarray(rois, np.int64).reshape(-1, 6)
    return np.array([box_label(box_counts(labels, b), ignore, dominant) for b in rois], np.uint8)


def ties(labels, rois, ignore=()):
    """(n,) bool: the maximum of c is reached by more than one label (clause 2 decides by order)."""
    rois = np.asarray(rois, np.int64).reshape(-1, 6)
    out = np.zeros(len(rois), bool)
    for i, b in enumerate(rois):
        c = box_counts(labels, b).copy()
        c[sorted(set(int(v) for v in ignore))] = 0
        out[i] = c.max() > 0 and np.count_nonzero(c == c.max()) > 1
    return out


# ---- the dense form: every box of one size at once ----------------------------------------------
def _window_sums(indicator, size):
    """(nz-sz+1, ny-sy+1, nx-sx+1) int64: the sum of `indicator` over the box with corner (z, y, x),
    from the 3-D cumulative sum (the eight corners of the integral image)."""
    sx, sy, sz = size
    nz, ny, nx = indicator.shape
    total = np.zeros((nz + 1, ny + 1, nx + 1), np.int64)
    total[1:, 1:, 1:] = indicator.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    return (total[sz:, sy:, sx:] - total[:-sz, sy:, sx:] - total[sz:, :-sy, sx:] - total[sz:, sy:, :-sx]
            + total[:-sz, :-sy, sx:] + total[:-sz, sy:, :-sx] + total[sz:, :-sy, :-sx] - total[:-sz, :-sy, :-sx])


def _dense_votes(labels, size, ignore):
    """The values that occur and are not ignored, ascending, and their box counts at every fitting
    box corner: (values, (len(values), nz-sz+1, ny-sy+1, nx-sx+1) int64)."""
    G = set(int(v) for v in ignore)
    values = [int(v) for v in np.unique(labels) if int(v) not in G]
    nz, ny, nx = labels.shape
    votes = np.zeros((len(values), nz - size[2] + 1, ny - size[1] + 1, nx - size[0] + 1), np.int64)
    for i, v in enumerate(values):
        votes[i] = _window_sums(labels == v, size)
    return np.array(values, np.int64), votes


def _dense_select(field, gen_mask, size):
    """The entries of a per-corner field at the centres (corner + size // 2) with gen_mask != 0, in
    raster order of the centres."""
    hx, hy, hz = (int(s) // 2 for s in size)
    nz, ny, nx = field.shape
    on = np.asarray(gen_mask)[hz:hz + nz, hy:hy + ny, hx:hx + nx] != 0
    return field[on]                    # boolean indexing walks z, y, x


def _dense_args(labels, gen_mask, size):
    labels, gen_mask = np.asarray(labels), np.asarray(gen_mask)
    assert labels.dtype == np.uint8 and labels.ndim == 3 and gen_mask.shape == labels.shape
    size = tuple(int(s) for s in size)
    assert len(size) == 3 and min(size) >= 1
    fits = all(s <= n for s, n in zip(size, labels.shape[::-1]))
    return labels, gen_mask, size, fits


def dense_labels(labels, gen_mask, size, ignore=(), dominant=-1):
    """(n,) uint8: the label of the box of `size` = (sx, sy, sz) around every voxel with
    gen_mask != 0 whose box [c - size // 2, c - size // 2 + size) fits the volume, raster order."""
    labels, gen_mask, size, fits = _dense_args(labels, gen_mask, size)
    if not fits:
        return np.zeros(0, np.uint8)
    G = sorted(set(int(v) for v in ignore))
    values, votes = _dense_votes(labels, size, G)
    out = np.full(votes.shape[1:], G[0] if G else 0, np.int64)                   # clause 3
    if len(values):
        top = votes.max(axis=0)
        out = np.where(top > 0, values[votes.argmax(axis=0)], out)                # clause 2: argmax takes the first
    if dominant >= 0:                                                             # clause 1
        out = np.where(_window_sums(labels == dominant, size) > 0, dominant, out)
        if dominant in G:
            out[...] = dominant
    return _dense_select(out, gen_mask, size).astype(np.uint8)


def dense_ties(labels, gen_mask, size, ignore=()):
    """(n,) bool for the regions of dense_labels: clause 2 decides by order."""
    labels, gen_mask, size, fits = _dense_args(labels, gen_mask, size)
    if not fits:
        return np.zeros(0, bool)
    _, votes = _dense_votes(labels, size, ignore)
    if not len(votes):
        return np.zeros(len(_dense_select(np.zeros(votes.shape[1:]), gen_mask, size)), bool)
    top = votes.max(axis=0)
    return _dense_select((top > 0) & ((votes == top).sum(axis=0) > 1), gen_mask, size)
