"""CPU checks of tests/coverage_oracle.py itself: the census is the DenseHistogram over the distinct
values (tests/stats_oracle.py, the restatement of Statistics/DenseHistogram.h), the painted coverage
equals a per-voxel count, and the round ends are the partial sums of the reference's list."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_oracle as V  # noqa: E402
import stats_oracle as S  # noqa: E402


def _values(seed, n):
    rng = np.random.default_rng(seed)
    v = rng.integers(-4, 5, n).astype(np.float32) * np.float32(0.25)
    v[rng.random(n) < 0.1] = np.float32(-0.0)
    v[rng.random(n) < 0.05] = np.float32(1e-41)     # a denormal
    v[rng.random(n) < 0.05] = np.float32(np.inf)
    v[rng.random(n) < 0.05] = np.float32(-np.inf)
    return v


def test_the_census_is_the_dense_histogram_over_the_distinct_values():
    for seed in range(5):
        v = _values(seed, 997)
        uniq, counts, n_nan = V.value_census(v)
        assert n_nan == 0 and uniq.dtype == np.float32 and counts.dtype == np.uint32
        assert (np.diff(uniq.astype(np.float64)) > 0).all()
        hist = S.lower_bound_counts(uniq, v)
        assert hist.size == uniq.size + 1 and hist[-1] == 0
        assert np.array_equal(hist[:-1], counts) and int(counts.sum()) == v.size


def test_census_zeros_nans_and_denormals():
    nan_pos, nan_neg = np.uint32(0x7fc00001).view(np.float32), np.uint32(0xffc00000).view(np.float32)
    d1, d2 = np.uint32(1).view(np.float32), np.uint32(2).view(np.float32)
    v = np.array([0.0, -0.0, nan_pos, d2, -0.0, nan_neg, d1, np.inf, -np.inf, nan_pos, d1], np.float32)
    uniq, counts, n_nan = V.value_census(v)
    assert n_nan == 3
    assert list(uniq.view(np.uint32)) == [0xff800000, 0, 1, 2, 0x7f800000]
    assert list(counts) == [1, 3, 2, 1, 1]
    uniq, counts, n_nan = V.value_census(np.array([nan_pos, nan_neg], np.float32))
    assert uniq.size == 0 and counts.size == 0 and n_nan == 2


def test_threshold_is_inclusive_and_takes_no_nan():
    d = np.uint32(5).view(np.float32)
    img = np.array([-1.0, -0.0, 0.0, d, 1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
    assert list(V.threshold_mask(img, 0.0, 1.0)[0]) == [0, 1, 1, 1, 1, 0, 0, 0, 0]
    assert list(V.threshold_mask(img, d, d)[0]) == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert list(V.threshold_mask(img, -np.inf, np.inf)[0]) == [1, 1, 1, 1, 1, 1, 0, 1, 1]
    m, c = V.threshold_mask(img.reshape(3, 3), -0.0, -0.0)
    assert m.shape == (3, 3) and c == 2


def test_painting_equals_a_count_voxel_by_voxel():
    rng = np.random.default_rng(3)
    shape = (3, 5, 37)
    mask = (rng.random(shape) < 0.4).astype(np.uint8)
    rois = []
    for _ in range(14):
        s = [int(rng.integers(1, n + 1)) for n in shape[::-1]]
        rois.append([int(rng.integers(0, n - e + 1)) for n, e in zip(shape[::-1], s)] + s)
    rois.append(rois[3])
    ends = [0, 1, 1, 4, 9, 15]
    got, want = V.roi_coverage(mask, rois, ends), V.roi_coverage_brute(mask, rois, ends)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert got[0][0] == 0 and got[0][1] == got[0][2] == np.prod(rois[0][3:])
    assert (np.diff(got[0]) >= 0).all() and (got[1] <= np.minimum(got[0], got[2])).all()


def test_round_ends_are_the_partial_sums_of_the_reference_list():
    assert V.SAMPLES_PER_ROUND == (10, 10, 10, 10, 10, 50, 100, 100, 100, 100, 500, 1000)
    assert V.ROUND_ENDS == tuple(itertools.accumulate(V.SAMPLES_PER_ROUND)) and V.ROUND_ENDS[-1] == 2000


def test_printed_lines():
    uniq, counts, _ = V.value_census(np.array([2.5, -0.0, 2.5, 1e-41], np.float32))
    assert V.census_lines(uniq, counts) == ["(-1e+12,0]\t|\t(0,9.99967e-42]\t|\t(9.99967e-42,2.5]\t|\t(2.5,inf)\t|\t",
                                            "1\t|\t1\t|\t2\t|\t0\t|\t"]
    assert V.coverage_lines([75], [25], 300, [10]) == ["Visited 75 voxels. 10 ROIs overlap 25/300 = 0.0833333"]
