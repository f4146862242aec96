"""tests/labels_oracle.py against hand-made boxes: every clause of the label rule with the expected
answer written as a literal (no GPU)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import labels_oracle as L  # noqa: E402


def box(*runs):
    """A (1, 1, n) label volume made of (label, count) runs, and the box that covers it."""
    flat = np.concatenate([np.full(c, v, np.uint8) for v, c in runs])
    return flat.reshape(1, 1, -1), [(0, 0, 0, flat.size, 1, 1)]


def one(runs, ignore=(), dominant=-1):
    vol, rois = box(*runs)
    got = L.roi_labels(vol, rois, ignore, dominant)
    assert got.dtype == np.uint8 and got.shape == (1,)
    return int(got[0])


def test_unique_maximum():
    assert one([(7, 2), (1, 5), (128, 3)]) == 1


def test_two_way_tie_takes_the_smaller_label():
    assert one([(7, 4), (2, 4), (0, 1)]) == 2
    vol, rois = box((7, 4), (2, 4), (0, 1))
    assert L.ties(vol, rois).tolist() == [True]
    assert L.ties(*box((7, 4), (2, 3))).tolist() == [False]


def test_tie_between_200_and_255():
    assert one([(255, 3), (200, 3), (1, 2)]) == 200


def test_dominant_present_with_a_single_voxel():
    assert one([(1, 9), (7, 1)], dominant=7) == 7


def test_dominant_absent():
    assert one([(1, 9), (2, 1)], dominant=7) == 1


def test_dominant_ignored_and_absent_still_wins():
    # the reference inserts the ignored labels into its map before it asks for the dominant one
    assert one([(1, 9), (2, 1)], ignore=(7,), dominant=7) == 7
    assert one([(1, 9), (7, 1)], ignore=(7,), dominant=7) == 7


def test_all_voxels_ignored_gives_the_smallest_ignored_label():
    assert one([(5, 3), (9, 4)], ignore=(9, 5, 3)) == 3
    assert one([(5, 3), (9, 4)], ignore=(9, 5, 9)) == 5


def test_an_ignored_label_that_would_have_been_the_mode():
    assert one([(0, 8), (2, 1), (1, 2)], ignore=(0,)) == 1
    assert one([(0, 8), (2, 1), (1, 2)]) == 0


def test_boxes_inside_a_volume():
    vol = np.zeros((3, 4, 5), np.uint8)
    vol[1:, :, 3:] = 200
    vol[0, 0, 0] = 255
    rois = [(0, 0, 0, 5, 4, 3), (3, 0, 1, 2, 4, 2), (0, 0, 0, 1, 1, 1), (2, 0, 1, 2, 1, 1)]
    assert L.roi_labels(vol, rois).tolist() == [0, 200, 255, 0]      # the last box ties 0 with 200
    assert L.ties(vol, rois).tolist() == [False, False, False, True]
    assert L.roi_labels(vol, rois, ignore=(0,), dominant=255).tolist() == [255, 200, 255, 200]


# ---- dense_labels (cumulative sums, all boxes at once) against roi_labels (a bincount per box) ----
DENSE_SHAPE = (7, 8, 11)
DENSE_SIZES = [(5, 3, 3), (4, 2, 6), (1, 1, 1), (11, 8, 7)]
DENSE_RULES = [((), -1), ((0,), -1), ((0, 200), 7),
               ((), 7),                          # a dominant label that occurs
               ((2,), 3),                        # one that does not occur
               ((7, 1), 7), ((3, 1), 3),         # a dominant label that is ignored too: occurring or not
               ((0, 1, 2, 7, 200), -1),          # every value ignored
               ((9, 0, 1, 2, 7, 200), 3)]


def generator_boxes(gen, size):
    """DenseROIGenerator's rule, centre by centre."""
    sx, sy, sz = size
    nz, ny, nx = gen.shape
    boxes = []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                x0, y0, z0 = x - sx // 2, y - sy // 2, z - sz // 2
                if gen[z, y, x] != 0 and min(x0, y0, z0) >= 0 and x0 + sx <= nx and y0 + sy <= ny and z0 + sz <= nz:
                    boxes.append((x0, y0, z0, sx, sy, sz))
    return np.array(boxes, np.int64).reshape(-1, 6)


def dense_volume():
    rng = np.random.default_rng(81)
    lab = np.array([0, 1, 2, 7, 200], np.uint8)[rng.integers(0, 5, (4, 4, 6))]
    lab = np.repeat(np.repeat(np.repeat(lab, 2, 0), 2, 1), 2, 2)[:7, :8, :11]      # blocks of 2 x 2 x 2
    lab[rng.integers(0, 7, 20), rng.integers(0, 8, 20), rng.integers(0, 11, 20)] = 1
    gen = (rng.integers(0, 4, DENSE_SHAPE) != 0).astype(np.uint16) * 300
    gen[3, 4, 5] = 1                                   # the centre of the whole-volume box
    assert lab.shape == DENSE_SHAPE and set(np.unique(lab)) == {0, 1, 2, 7, 200}
    return np.ascontiguousarray(lab), gen


def test_dense_labels_equal_roi_labels_on_the_generators_boxes():
    lab, gen = dense_volume()
    for size in DENSE_SIZES:
        boxes = generator_boxes(gen, size)
        assert len(boxes) == {(11, 8, 7): 1, (1, 1, 1): np.count_nonzero(gen)}.get(size, len(boxes)) > 0
        for ignore, dominant in DENSE_RULES:
            got = L.dense_labels(lab, gen, size, ignore, dominant)
            assert got.dtype == np.uint8 and got.shape == (len(boxes),)
            assert np.array_equal(got, L.roi_labels(lab, boxes, ignore, dominant)), (size, ignore, dominant)
        for ignore in [(), (0,), (0, 200), (0, 1, 2, 7, 200)]:
            t = L.dense_ties(lab, gen, size, ignore)
            assert t.dtype == bool and np.array_equal(t, L.ties(lab, boxes, ignore)), (size, ignore)
    t = L.dense_ties(lab, gen, (5, 3, 3))
    assert t.any() and not t.all()                     # the comparison above saw both


def test_dense_labels_every_clause_is_taken():
    lab, gen = dense_volume()
    size = (4, 2, 6)
    plain = L.dense_labels(lab, gen, size)
    assert len(set(plain.tolist())) > 2
    with7 = L.dense_labels(lab, gen, size, (), 7)
    assert (with7 != plain).any() and (with7 == plain).any() and set(with7[with7 != plain].tolist()) == {7}
    assert np.array_equal(L.dense_labels(lab, gen, size, (2,), 3), L.dense_labels(lab, gen, size, (2,)))
    assert set(L.dense_labels(lab, gen, size, (3, 1), 3).tolist()) == {3}
    assert set(L.dense_labels(lab, gen, size, (200, 0, 1, 2, 7)).tolist()) == {0}
    assert set(L.dense_labels(lab, gen, size, (200, 1, 2, 7, 0, 9), 3).tolist()) == {0}


def test_dense_labels_box_larger_than_the_volume_and_an_empty_mask():
    lab, gen = dense_volume()
    assert L.dense_labels(lab, gen, (12, 3, 3)).shape == (0,) and L.dense_ties(lab, gen, (3, 3, 8)).shape == (0,)
    none = L.dense_labels(lab, np.zeros_like(gen), (5, 3, 3), (0,), 7)
    assert none.dtype == np.uint8 and none.shape == (0,)
