"""The rule of ife_roi_labels / ife_dense_roi_labels (include/ife_hip.h) in numpy.

For one box of a uint8 label volume, a set G of ignored labels and a dominant label d (-1: none):
n(l) = the number of voxels of the box that carry l, c(l) = 0 if l is in G, else n(l).

  1. d >= 0 and (n(d) > 0 or d in G): the label is d
  2. else max c > 0: the smallest l with c(l) = max c
  3. else: the smallest member of G

Where the maximum is unique this is tools/ExtractLabels.cxx:164-212; at ties the reference has no
defined answer (it takes whichever key its unordered_map iterates first), so "smallest" is ours.
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
