"""tests/region_oracle.py against cases written out by hand: the oracle is what the device results
are held equal to, so it is checked on its own first."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_oracle as R  # noqa: E402


def test_bounding_box_by_hand():
    m = np.zeros((4, 5, 6), np.uint8)
    assert R.bounding_box(m) == ((0, 0, 0), (0, 0, 0), 0)
    m[1, 2, 3] = 7
    assert R.bounding_box(m) == ((3, 2, 1), (1, 1, 1), 1)
    m[3, 0, 5] = 1
    assert R.bounding_box(m) == ((3, 0, 1), (3, 3, 3), 2)
    assert R.bounding_box(np.ones((4, 5, 6), np.uint16)) == ((0, 0, 0), (6, 5, 4), 120)


def test_foreground_rules():
    u = np.array([[[0, 256, 1]]], np.uint16)
    assert R.foreground(u).tolist() == [[[False, True, True]]]
    i = np.array([[[0, -1, -32768]]], np.int16)
    assert R.foreground(i).tolist() == [[[False, True, True]]]
    f = np.array([[[0.0, -0.0, 1e-45, np.nan, -np.inf]]], np.float32)   # 1e-45: the smallest denormal
    assert R.foreground(f).tolist() == [[[False, False, True, True, True]]]


def test_extract_region_by_hand():
    src = np.arange(2 * 3 * 4, dtype=np.int16).reshape(2, 3, 4)
    assert np.array_equal(R.extract_region(src, (1, 1, 0), (2, 2, 1)), [[[5, 6], [9, 10]]])
    got = R.extract_region(src, (-1, 2, 1), (3, 2, 1), pad_value=-7)
    assert np.array_equal(got, [[[-7, 20, 21], [-7, -7, -7]]])
    assert np.array_equal(R.extract_region(src, (9, 0, 0), (2, 1, 1), pad_value=3), [[[3, 3]]])
    # flips: x reverses inside rows, z the order of the planes; the pad moves with them
    got = R.extract_region(src, (-1, 2, 1), (3, 2, 1), pad_value=-7, flip=(True, False, False))
    assert np.array_equal(got, [[[21, 20, -7], [-7, -7, -7]]])
    got = R.extract_region(src, (-1, 2, 1), (3, 2, 1), pad_value=-7, flip=(False, True, False))
    assert np.array_equal(got, [[[-7, -7, -7], [-7, 20, 21]]])
    got = R.extract_region(src, (0, 0, 0), (1, 1, 2), flip=(False, False, True))
    assert np.array_equal(got, [[[12]], [[0]]])
    assert got.dtype == src.dtype and got.flags.c_contiguous
    with pytest.raises(AssertionError):
        R.extract_region(src, (-1, 0, 0), (2, 1, 1))


def test_constant_pad_is_a_region():
    src = np.arange(6, dtype=np.uint8).reshape(1, 2, 3)
    lower, upper = (1, 2, 0), (2, 0, 0)
    got = R.extract_region(src, [-v for v in lower], [n + l + u for n, l, u in zip((3, 2, 1), lower, upper)], 9)
    want = np.pad(src, ((0, 0), (2, 0), (1, 2)), constant_values=9)
    assert np.array_equal(got, want)


def test_axis_split_by_hand():
    assert R.axis_split(2, 3, 10, False) == (0, 3, 0, 2, 1)
    assert R.axis_split(-2, 5, 10, False) == (2, 3, 0, 0, 1)
    assert R.axis_split(8, 5, 10, False) == (0, 2, 3, 8, 1)
    assert R.axis_split(8, 5, 10, True) == (3, 2, 0, 9, -1)
    assert R.axis_split(-2, 14, 10, True) == (2, 10, 2, 9, -1)
    assert R.axis_split(10, 2, 10, False) == (2, 0, 0, 0, 1)
    assert R.axis_split(-2, 2, 10, True) == (2, 0, 0, 0, -1)


def test_label_membership_by_hand():
    lab = np.array([0, 1, 2, 255, 256, 65535], np.uint16)
    assert R.label_membership(lab, [255, 256]).tolist() == [0, 0, 0, 1, 1, 0]
    assert R.label_membership(lab, [2, 0, 2], inside=7, outside=65535).tolist() == [7, 65535, 7, 65535, 65535, 65535]
    assert R.label_membership(lab, []).tolist() == [0] * 6
    assert R.label_membership(lab.astype(np.uint8), [0]).dtype == np.uint8


def test_geometry_shift_by_hand():
    assert R.shift_origin((1.0, 2.0, 3.0), (0.5, 2.0, 1.0), (2, -1, 4)).tolist() == [2.0, 0.0, 7.0]
    srow = np.array([[0, 2, 0, 10], [-3, 0, 0, 20], [0, 0, 1, 30]], np.float32)
    assert R.shift_srow(srow, (1, 2, 3)).tolist() == [14.0, 17.0, 33.0]
    assert np.allclose(R.quaternion_rotation(0, 0, 1), np.diag([-1.0, -1.0, 1.0]))
    assert R.shift_qoffset((0, 0, 0), -1.0, (0.5, 2.0, 1.5), (1, 1, 1), (2, 3, 4)).tolist() == [2.0, 7.0, -5.0]
    assert R.within_one_ulp(np.float32(0.1), 0.1)
    assert R.within_one_ulp(np.nextafter(np.float32(0.1), np.float32(1)), 0.1)
    assert not R.within_one_ulp(np.float32(0.1) + np.float32(3e-8), 0.1)
