"""tests/stats_oracle.py against the project's oracle, on the CPU: the checker of
tests/test_gpu_stats_seams.py is held equal to `oracle.sort_f32`, `oracle.dense_histogram`,
`oracle.equalized_edges` and `oracle.roi_histograms`, and its constants to csrc/stats_kernels.hpp."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stats_oracle as so  # noqa: E402


def test_constants_are_those_of_the_header():
    k = so.kernel_constants()
    assert k == {"SORT_THREADS": so.SORT_THREADS, "SORT_KPT": so.SORT_KPT, "SORT_SUB": so.SORT_SUB,
                 "SORT_SEGS": so.SORT_SEGS, "HIST_MAX_EDGES": so.HIST_MAX_EDGES,
                 "ROI_SPLIT": so.ROI_SPLIT, "ROI_MAX_LDS_WORDS": so.ROI_MAX_LDS_WORDS}
    assert so.SORT_TILE == 16384 and so.SORT_SUBTILE == 4096
    assert so.sort_geometry(16 * 16384) == (16, 1) and so.sort_geometry(16 * 16384 + 1) == (17, 2)


def test_keys_round_trip_and_order():
    v = np.concatenate([so.SPECIALS, so.mixed_column(5000, 1)])
    k = so.keys(v)
    assert k.dtype == np.uint32
    assert so.same_bits(so.from_keys(k), v)                      # every special value, bit for bit
    edge = np.array([0x007FFFFF, 0x00800000, 0x7FFFFFFF, 0x80000000, 0xFF7FFFFF, 0xFF800000], np.uint32)
    f = so.from_keys(edge)                                       # -inf, -FLT_MAX, -0, +0, FLT_MAX, +inf
    assert f.tolist() == [-np.inf, -3.4028234663852886e38, 0.0, 0.0, 3.4028234663852886e38, np.inf]
    assert np.signbit(f).tolist() == [True, True, True, False, False, False]
    assert np.array_equal(so.keys(f), edge)
    # the key order is the value order, with -0 strictly below +0
    a, b = v[:, None], v[None, :]
    lt = (a < b) | ((a == 0) & (b == 0) & np.signbit(a) & ~np.signbit(b))
    assert np.array_equal(k[:, None] < k[None, :], lt)


def test_assert_no_nan():
    so.assert_no_nan(so.SPECIALS)
    with pytest.raises(AssertionError):
        so.sorted_bits(np.array([1.0, np.nan], np.float32))


@pytest.mark.parametrize("n", [0, 1, 2, 70001])
def test_sorted_bits_against_oracle(oracle, n):
    v = so.mixed_column(n, 10 + n)
    got = so.sorted_bits(v)
    assert np.array_equal(got, oracle.sort_f32(v))                # by value: qsort leaves +-0 unordered
    assert np.array_equal(np.sort(got.view(np.uint32)), np.sort(v.view(np.uint32)))
    z = got[got == 0]
    assert z.size == 0 or np.all(np.diff(np.signbit(z).astype(int)) <= 0)   # every -0 before every +0


def test_sorted_bits_on_special_values(oracle):
    rng = np.random.default_rng(3)
    v = np.concatenate([np.tile(so.SPECIALS, 50), rng.integers(-3, 4, 2000).astype(np.float32),
                        -np.zeros(300, np.float32)])
    rng.shuffle(v)
    got = so.sorted_bits(v)
    assert np.array_equal(got, oracle.sort_f32(v))
    assert np.all(np.diff(so.keys(got).astype(np.int64)) >= 0)


def test_lower_bound_counts_against_oracle(oracle):
    rng = np.random.default_rng(4)
    edges = np.sort(np.round(rng.normal(0, 3, 200), 1).astype(np.float32))   # duplicate edges happen
    assert np.unique(edges).size < edges.size
    v = np.round(rng.normal(0, 4, 50000), 1).astype(np.float32)              # values on edges happen
    assert np.isin(v, edges).sum() > 1000
    c, _ = oracle.dense_histogram(edges, v)
    assert np.array_equal(so.lower_bound_counts(edges, v), c)
    inf = np.array([np.inf, -np.inf, 0.0, -0.0], np.float32)
    c, _ = oracle.dense_histogram([-np.inf, 0.0, np.inf], inf)
    assert np.array_equal(so.lower_bound_counts([-np.inf, 0.0, np.inf], inf), c) and c.tolist() == [1, 2, 1, 0]
    # a NaN compares false with every edge: lower_bound stops at the first one
    assert so.lower_bound_counts([1.0, 2.0], [np.nan, 1.5, 5.0]).tolist() == [1, 1, 1]
    c, _ = oracle.dense_histogram([1.0, 2.0], [np.nan, 1.5, 5.0])
    assert c.tolist() == [1, 1, 1]


def test_walk_against_oracle_on_the_random_draws(oracle):
    kinds = {0: 0, 1: 0, 3: 0}
    for v, nb in so.edge_draws():
        st, e = so.walk(v, nb)
        kinds[st] += 1
        try:
            want = oracle.equalized_edges(v, nb)
        except oracle.EdgeWalkError as err:
            assert st == err.rc
            continue
        assert st == 0 and so.same_bits(e, want)
        st64, e64 = so.walk(v.astype(np.float64), nb)
        assert st64 == 0 and np.array_equal(e64, oracle.equalized_edges(v.astype(np.float64), nb))
    # what test_edges_random_against_oracle_and_compiled_reference asserts of the same draws
    assert kinds[0] > 150 and kinds[1] > 0 and kinds[3] > 0, kinds


def test_walk_known_answers(oracle):
    assert so.walk(np.arange(1, 10, dtype=np.float64), 3)[1].tolist() == [4.0, 7.0]
    st, e = so.walk(np.array([1, 1, 1, 1, 1, 2, 2, 3, 3, 3], np.float32), 3)
    assert st == 0 and e.tolist() == [2.0, 3.0]
    assert so.walk(np.ones(8), 2)[1].tolist() == [1.0]
    assert so.walk(np.arange(1, 10), 10)[0] == 1
    st, e = so.walk(np.arange(5.0), 1)
    assert st == 0 and e.size == 0


def test_walk_runs_past_the_end(oracle):
    for dt in (np.float32, np.float64):
        v = np.array(so.RC3_VALUES, dt)
        assert so.walk(v, so.RC3_BINS)[0] == 3
        with pytest.raises(oracle.EdgeWalkError) as ei:
            oracle.equalized_edges(v, so.RC3_BINS)
        assert ei.value.rc == 3


def test_coordinate_counts_against_oracle(oracle):
    rng = np.random.default_rng(6)
    shape = (7, 5, 9)
    feat, edges = so.coordinate_features(shape), so.coordinate_edges(shape)
    assert feat[3, 2, 8].tolist() == [8.0, 2.0, 3.0] and edges.shape == (3, 9)
    mask = (rng.random(shape) < 0.7).astype(np.uint8)
    mask[4] = 0
    rois = [[0, 0, 0, 9, 5, 7], [2, 1, 3, 4, 3, 4], [8, 4, 6, 1, 1, 1], [1, 1, 4, 3, 3, 1], [1, 1, 1, 0, 2, 2]]
    for m in (np.ones(shape, np.uint8), mask):
        want, _ = oracle.roi_histograms(feat, m, rois, edges)
        got = so.coordinate_counts(m, rois)
        assert np.array_equal(got, want)
        assert got[3].sum() == (0 if m is mask else 27) and got[4].sum() == 0
    full = so.coordinate_counts(np.ones(shape, np.uint8), rois[:1])[0]
    assert full[2].tolist() == [45] * 7 + [0] * 3 and full[0].tolist() == [35] * 9 + [0]
