"""Per-region label modes on the device (ife_roi_labels, ife_dense_roi_labels): the mode of a
uint8 label volume inside every box, under ignored labels and a dominant label.

The checker is tests/labels_oracle.py (a bincount per box, then the three clauses of the rule);
for the dense form the box-list call on the boxes of the generator's rule is the second witness.
These are integers: everything must be EQUAL.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import labels_oracle as L  # noqa: E402
from test_gpu_dense_bag import dense_boxes  # noqa: E402  (the generator's rule in numpy)

pytestmark = pytest.mark.gpu

SHAPE = (9, 11, 70)             # a row is two 64-voxel segments, boxes straddle the seam
SIZES = [(5, 3, 3), (4, 2, 6), (1, 1, 1), (70, 11, 9)]
IGNORES = [(), (0,), (0, 255), (2, 2)]
DOMINANTS = [-1, 7, 0, 3]       # 3 does not occur
RULES = [(g, d) for g in IGNORES for d in DOMINANTS]


def base_labels():
    """Slabs and blocks of {0, 1, 2, 7, 128, 200, 255} and a sprinkle of single voxels of any
    value but 3."""
    rng = np.random.default_rng(71)
    lab = np.zeros(SHAPE, np.uint8)
    lab[:, :, 10:30] = 1
    lab[:, :, 30:52] = 2
    lab[:, :, 52:66] = 200
    lab[:, :, 66:] = 255            # the slab 200 | 255 ends in the second row segment
    lab[:, 4:8, 60:68] = 128        # a block across the seam at x = 64
    lab[2:6, 2:9, 20:40] = 7
    lab[6:, :5, :12] = 255
    pos = rng.choice(lab.size, 320, replace=False)
    val = rng.integers(0, 256, pos.size)
    val[val == 3] = 4
    lab.reshape(-1)[pos] = val
    assert not (lab == 3).any()
    return lab


def gen_mask(dtype):
    rng = np.random.default_rng(72)
    on = rng.integers(0, 5, SHAPE) < 3
    on[4, 5, 35] = True             # the centre of the whole-volume box
    return on.astype(dtype) * (3 if dtype == np.uint8 else 700)


def hand_boxes():
    """Boxes that touch every face of the volume, one across the seam, the whole volume."""
    nz, ny, nx = SHAPE
    return np.array([(0, 2, 3, 7, 4, 2), (nx - 6, 1, 1, 6, 3, 5), (20, 0, 2, 9, 2, 4), (31, ny - 3, 0, 12, 3, 3),
                     (40, 3, 0, 5, 5, 1), (12, 4, nz - 2, 30, 2, 2), (58, 2, 1, 12, 8, 7), (0, 0, 0, nx, ny, nz),
                     (0, 0, 0, 1, 1, 1), (nx - 1, ny - 1, nz - 1, 1, 1, 1)], np.int64)


@pytest.fixture(scope="module")
def base():
    """The base volume and, per box size, the generator's boxes and the 256 counts of every box:
    computed once, shared, never written to."""
    lab = base_labels()
    gen = gen_mask(np.uint8)
    case = {"labels": lab, "gen": gen, "boxes": {}, "counts": {}}
    for size in SIZES + ["hand"]:
        boxes = hand_boxes() if size == "hand" else dense_boxes(gen, size)
        counts = np.stack([L.box_counts(lab, b) for b in boxes])
        for a in (boxes, counts):
            a.setflags(write=False)
        case["boxes"][size], case["counts"][size] = boxes, counts
    lab.setflags(write=False)
    gen.setflags(write=False)
    return case


def want(case, size, ignore, dominant):
    return np.array([L.box_label(c, ignore, dominant) for c in case["counts"][size]], np.uint8)


def test_the_base_volume_has_ties_and_unique_maxima(base):
    lab = base["labels"]
    assert set(np.unique(lab)) >= {0, 1, 2, 7, 128, 200, 255}
    for size in [(5, 3, 3), (4, 2, 6)]:
        t = L.ties(lab, base["boxes"][size])
        assert t.any() and not t.all(), size
    assert len(base["boxes"][(70, 11, 9)]) == 1 and len(base["boxes"][(1, 1, 1)]) > 3000


# ---- ife_roi_labels ----------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + ["hand"], ids=str)
def test_roi_labels_match_the_oracle(ctx, base, size):
    boxes = base["boxes"][size]
    for ignore, dominant in RULES:
        got = ctx.roi_labels(base["labels"], boxes, ignore, dominant)
        assert got.dtype == np.uint8 and got.shape == (len(boxes),)
        assert np.array_equal(got, want(base, size, ignore, dominant)), (ignore, dominant)
    assert np.array_equal(want(base, size, (), -1), L.roi_labels(base["labels"], boxes))


def test_roi_labels_refusals(ctx, ife, base):
    lib = ife.load_library()
    lab = base["labels"]
    d = ife._desc(lab.shape, (1.0, 1.0, 1.0))
    nz, ny, nx = SHAPE

    def call(rois, n=None, ignore=(), dominant=-1, dtype=ife.U8):
        rois = np.ascontiguousarray(rois, np.int64).reshape(-1, 6)
        out = np.full(max(len(rois), 1), 77, np.uint8)
        ign = (C.c_int * len(ignore))(*ignore) if ignore else None
        rc = lib.ife_roi_labels(ctx._h, lab.ctypes.data, dtype, C.byref(d), rois.ctypes.data,
                                len(rois) if n is None else n, ign, len(ignore), dominant, out.ctypes.data,
                                ife.MEM_HOST)
        return rc, out

    good = (1, 1, 1, 3, 3, 3)
    for bad in [(nx - 2, 0, 0, 3, 1, 1), (0, ny - 1, 0, 1, 2, 1), (0, 0, nz, 1, 1, 1), (-1, 0, 0, 2, 2, 2),
                (0, 0, 0, 0, 1, 1), (0, 0, 0, 1, 1, -1)]:
        rc, out = call([good, bad])
        assert rc == ife.E_ARG and np.all(out == 77), bad        # out is untouched
    assert call([good], dtype=ife.U16)[0] == ife.E_ARG
    assert call([good], ignore=(0, 256))[0] == ife.E_ARG
    assert call([good], ignore=(-1,))[0] == ife.E_ARG
    assert call([good], dominant=256)[0] == ife.E_ARG
    rc, out = call([good], n=0)
    assert rc == ife.OK and np.all(out == 77)                     # n_rois = 0: accepted, nothing written
    assert ctx.roi_labels(lab, np.zeros((0, 6), np.int64)).shape == (0,)
    rc, out = call([good], dominant=-5)                           # any negative value: no dominant label
    assert rc == ife.OK and out[0] == L.roi_labels(lab, [good])[0]


# ---- ife_dense_roi_labels ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_dense_roi_labels_match_oracle_and_box_list(ctx, base, size, dtype):
    gen = gen_mask(dtype)
    boxes = base["boxes"][size]
    assert np.array_equal(dense_boxes(gen, size), boxes)
    for ignore, dominant in RULES:
        got = ctx.dense_roi_labels(base["labels"], gen, size, ignore, dominant)
        assert got.dtype == np.uint8 and got.shape == (len(boxes),)
        assert np.array_equal(got, want(base, size, ignore, dominant)), (ignore, dominant)
        assert np.array_equal(got, ctx.roi_labels(base["labels"], boxes, ignore, dominant)), (ignore, dominant)


def test_dense_roi_labels_box_larger_than_the_volume(ctx, base):
    got = ctx.dense_roi_labels(base["labels"], base["gen"], (71, 3, 3))
    assert got.dtype == np.uint8 and got.shape == (0,)


def test_dense_roi_labels_count_only_and_capacity(ctx, ife, base):
    lib = ife.load_library()
    lab, gen, size = base["labels"], gen_mask(np.uint16), (4, 2, 6)
    n_want = len(base["boxes"][size])
    d = ife._desc(lab.shape, (1.0, 1.0, 1.0))

    def call(out, capacity):
        n = C.c_int64(-1)
        rc = lib.ife_dense_roi_labels(ctx._h, lab.ctypes.data, ife.U8, gen.ctypes.data, ife.U16, C.byref(d),
                                      ife._size_arg(size), None, 0, -1, None if out is None else out.ctypes.data,
                                      capacity, C.byref(n), ife.MEM_HOST)
        return rc, n.value

    assert call(None, 0) == (ife.OK, n_want) and n_want > 1
    small = np.full(n_want - 1, 77, np.uint8)
    assert call(small, len(small)) == (ife.E_SIZE, n_want)        # the count is still reported
    assert np.all(small == 77)                                    # and nothing was written
    full = np.full(n_want + 3, 77, np.uint8)
    assert call(full, len(full)) == (ife.OK, n_want)
    assert np.array_equal(full[:n_want], want(base, size, (), -1)) and np.all(full[n_want:] == 77)
    n = C.c_int64(-1)                                             # there is no mask to fall back on
    assert lib.ife_dense_roi_labels(ctx._h, lab.ctypes.data, ife.U8, None, ife.U8, C.byref(d), ife._size_arg(size),
                                    None, 0, -1, full.ctypes.data, len(full), C.byref(n), ife.MEM_HOST) == ife.E_ARG


# ---- all 256 values ----------------------------------------------------------------------------
def test_all_256_values(ctx):
    """Every value 0..255 eight times: 256 planes, more than the 255 codes one byte holds beside
    the value for "another group", so the dense call takes two groups whatever the budget."""
    rng = np.random.default_rng(73)
    lab = rng.permutation(np.arange(2048) % 256).astype(np.uint8).reshape(4, 8, 64)
    assert np.all(np.bincount(lab.ravel(), minlength=256) == 8)
    gen = np.ones(lab.shape, np.uint8)
    size = (3, 3, 3)
    boxes = dense_boxes(gen, size)
    assert len(boxes) == 62 * 6 * 2
    for ignore, dominant in [((), -1), ((0, 255), -1), ((), 255), (tuple(range(1, 256)), -1)]:
        ref = L.roi_labels(lab, boxes, ignore, dominant)
        assert np.array_equal(ctx.roi_labels(lab, boxes, ignore, dominant), ref), (ignore, dominant)
        assert np.array_equal(ctx.dense_roi_labels(lab, gen, size, ignore, dominant), ref), (ignore, dominant)


# ---- the labels in groups ----------------------------------------------------------------------
def test_dense_roi_labels_in_groups(ife, ctx, base):
    """IFE_OPT_DENSE_SCRATCH_MB = 1: scratch per group of bg labels is nvox * (1 + 3 * bg) bytes
    (include/ife_hip.h), so 1 MiB holds (2^20 - 6930) // (3 * 6930) = 50 labels of the 6930 voxels
    at a time and the labels of the base volume that take a plane go through in groups."""
    lab, gen, size = base["labels"], base["gen"], (5, 3, 3)
    nvox, budget = lab.size, 1 << 20
    assert nvox == 6930
    for ignore, dominant, n_planes, n_groups in [((), -1, 182, 4), ((0, 255), 7, 180, 4)]:
        planes = [v for v in np.unique(lab) if v not in ignore]   # occurs, not ignored (the dominant one goes last)
        assert len(planes) == n_planes
        assert nvox * (1 + 3 * min(len(planes), 255)) > budget
        bg = min((budget - nvox) // (3 * nvox), len(planes), 255)
        assert bg == 50 and math.ceil(len(planes) / bg) == n_groups >= 3
        with ife.Context(0) as c:
            c.set_option(ife.OPT_DENSE_SCRATCH_MB, 1)
            got = c.dense_roi_labels(lab, gen, size, ignore, dominant)
        assert np.array_equal(got, want(base, size, ignore, dominant))
        assert np.array_equal(got, ctx.dense_roi_labels(lab, gen, size, ignore, dominant))    # ungrouped


# ---- more boxes than the grid of the list kernel -----------------------------------------------
# csrc/labels_kernels.hpp LABELS_GRID_CAP: roi_labels_kernel runs min(n_rois, 16384) workgroups, a
# workgroup takes the boxes r, r + 16384, ...
def test_roi_labels_second_trip_of_the_capped_grid(ctx):
    rng = np.random.default_rng(74)
    lab = rng.integers(0, 3, (34, 32, 32)).astype(np.uint8)
    z, y, x = np.meshgrid(np.arange(0, 34, 2), np.arange(32), np.arange(32), indexing="ij")
    boxes = np.stack([x.ravel(), y.ravel(), z.ravel(), np.ones(x.size, int), np.ones(x.size, int),
                      np.full(x.size, 2)], 1).astype(np.int64)
    assert len(boxes) == 17408 > 16384
    a, b = lab[0::2].ravel(), lab[1::2].ravel()                   # the two voxels of every box
    ref = np.minimum(a, b)                                        # one label, or a tie the smaller one takes
    assert np.count_nonzero(a != b) > 5000
    got = ctx.roi_labels(lab, boxes)
    assert np.array_equal(got[:16384], ref[:16384])
    assert np.array_equal(got[16384:], ref[16384:])               # the second trip
    ref0 = np.where(a == 0, b, np.where(b == 0, a, ref))          # 0 ignored: the other voxel, 0 if both
    assert np.array_equal(ctx.roi_labels(lab, boxes, ignore=(0,)), ref0)


# ---- device-resident inputs and output ---------------------------------------------------------
def test_device_resident_labels(ctx, ife, base):
    import torch
    lib = ife.load_library()
    lab, size = base["labels"], (4, 2, 6)
    boxes = base["boxes"][size]
    gen = gen_mask(np.uint16)
    d = ife._desc(lab.shape, (1.0, 1.0, 1.0))
    d_lab = torch.from_numpy(np.array(lab)).cuda()
    d_gen = torch.from_numpy(gen.view(np.int16)).cuda()
    d_boxes = torch.from_numpy(np.array(boxes)).cuda()
    d_out = torch.full((len(boxes) + 5,), 77, dtype=torch.uint8, device="cuda")
    ign = (C.c_int * 2)(0, 255)
    torch.cuda.synchronize()
    ref = want(base, size, (0, 255), 7)
    assert lib.ife_roi_labels(ctx._h, d_lab.data_ptr(), ife.U8, C.byref(d), d_boxes.data_ptr(), len(boxes), ign, 2, 7,
                              d_out.data_ptr(), ife.MEM_DEVICE) == ife.OK
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:len(boxes)], ref) and np.all(got[len(boxes):] == 77)
    d_out.fill_(77)
    torch.cuda.synchronize()
    n = C.c_int64(-1)
    assert lib.ife_dense_roi_labels(ctx._h, d_lab.data_ptr(), ife.U8, d_gen.data_ptr(), ife.U16, C.byref(d),
                                    ife._size_arg(size), ign, 2, 7, d_out.data_ptr(), len(boxes) + 5, C.byref(n),
                                    ife.MEM_DEVICE) == ife.OK
    got = d_out.cpu().numpy()
    assert n.value == len(boxes) and np.array_equal(got[:len(boxes)], ref) and np.all(got[len(boxes):] == 77)
    # a device-resident box list is checked on the device before anything reads through it
    bad = np.array(boxes[:4])
    bad[2, 0] = SHAPE[2] - 1
    d_bad = torch.from_numpy(bad).cuda()
    d_out.fill_(77)
    torch.cuda.synchronize()
    assert lib.ife_roi_labels(ctx._h, d_lab.data_ptr(), ife.U8, C.byref(d), d_bad.data_ptr(), 4, None, 0, -1,
                              d_out.data_ptr(), ife.MEM_DEVICE) == ife.E_ARG
    assert np.all(d_out.cpu().numpy() == 77)
