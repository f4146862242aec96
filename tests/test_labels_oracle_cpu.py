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
