"""tests/bspline_oracle.py held to independent facts (no GPU): scipy's spline filter and
map_coordinates in mirror mode, the horizons re-derived from the poles, the partition of unity of
the weights, and interpolation at the samples.

The bound against scipy is 1e-9 * max|src|: the oracle truncates the causal start at 1e-10 per
pole and axis where the line is longer than the horizon, scipy sums further; everything else is
rounding."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bspline_oracle as B  # noqa: E402

ndimage = pytest.importorskip("scipy.ndimage")
ORDERS = (2, 3, 4, 5)


@pytest.mark.parametrize("order", ORDERS)
def test_prefilter_matches_scipy_on_every_line_length(order):
    rng = np.random.default_rng(order)
    worst = 0.0
    for n in range(2, 98):
        src = rng.standard_normal((n, 3)) * 1000
        got = B.filter_lines(src.copy(), order)
        want = ndimage.spline_filter1d(src, order, axis=0, mode="mirror", output=np.float64)
        worst = max(worst, np.abs(got - want).max() / np.abs(src).max())
    print("order %d: worst difference to scipy %.3g of max|src|" % (order, worst))
    assert worst <= 1e-9


def test_a_line_of_one_sample_is_untouched_and_low_orders_are_the_source():
    src = np.arange(5, dtype=np.float64).reshape(1, 5) - 2.5
    for order in ORDERS:
        assert np.array_equal(B.filter_lines(src.copy(), order), src)
    vol = np.random.default_rng(0).standard_normal((3, 4, 5)).astype(np.float32)
    for order in (0, 1):
        assert np.array_equal(B.coefficients(vol, order), vol.astype(np.float64))


def test_horizons_rederived():
    for order in ORDERS:
        assert len(B.poles(order)) == len(B.HORIZONS[order])
        for z, h in zip(B.poles(order), B.HORIZONS[order]):
            assert -1.0 < z < 0.0
            assert h == math.ceil(math.log(1e-10) / math.log(abs(z)))
    assert B.HORIZONS == {2: (14,), 3: (18,), 4: (23, 6), 5: (28, 8)}
    assert not B.poles(0) and not B.poles(1)


@pytest.mark.parametrize("order", range(6))
def test_weights_sum_to_one_and_match_the_basis(order):
    lo = -0.5 if order % 2 == 0 else 0.0
    w = np.concatenate([np.linspace(lo, lo + 1.0, 1001), [lo, lo + 1.0, lo + 0.5]])
    wt = B.weights(order, w)
    assert wt.shape == (order + 1, w.size)
    total = wt[0].copy()
    for k in range(1, order + 1):
        total = total + wt[k]
    assert np.abs(total - 1.0).max() <= 4 * np.finfo(np.float64).eps
    # the cardinal B-spline at the taps' distances, from its truncated-power form, whose own
    # alternating terms reach C(6, 3) * 3^5 / 5! = 40: its cancellation error is some 1e-14
    def basis(x):
        n, acc = order, np.zeros_like(x)
        for k in range(n + 2):
            acc = acc + (-1) ** k * math.comb(n + 1, k) * np.maximum(x + (n + 1) / 2.0 - k, 0.0) ** n
        return acc / math.factorial(n)
    if order > 0:
        for k in range(order + 1):
            assert np.abs(wt[k] - basis(w - (k - order // 2))).max() <= 1e-13


@pytest.mark.parametrize("order", ORDERS)
def test_whole_path_matches_map_coordinates(order):
    rng = np.random.default_rng(10 + order)
    src = rng.standard_normal((7, 6, 9)) * 1000
    sp, o = (0.7, 0.9, 2.5), (1.0, -2.0, 3.0)
    dshape, dsp, do = (11, 13, 17), (0.35, 0.38, 1.3), (1.1, -1.9, 3.2)
    got = B.resample(src, sp, o, dshape, dsp, do, order=order, default=-7.5)
    tabs = B.tables(order, src.shape, sp, o, dshape, dsp, do, (0, 0, 0))
    assert all(t[0].all() for t in tabs)                  # the comparison is about inside voxels
    cz, cy, cx = ((do[d] + np.arange(dshape[2 - d]) * dsp[d] - o[d]) / sp[d] for d in (2, 1, 0))
    grid = np.meshgrid(cz, cy, cx, indexing="ij")
    want = ndimage.map_coordinates(src, grid, order=order, mode="mirror", output=np.float64)
    worst = np.abs(got - want).max() / np.abs(src).max()
    print("order %d: worst difference to map_coordinates %.3g of max|src|" % (order, worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("order", range(6))
def test_interpolating_at_the_samples_returns_the_source(order):
    src = np.random.default_rng(20 + order).standard_normal((5, 19, 30)) * 1000
    sp, o = (0.75, 0.5, 2.5), (-3.25, 4.0, 1.5)
    got = B.resample(src, sp, o, src.shape, sp, o, order=order, default=-7.5)
    assert np.abs(got - src).max() <= 1e-9 * np.abs(src).max()
    flat = B.resample(src[:1], sp, o, (1,) + src.shape[1:], sp, o, order=order, default=-7.5)    # nz = 1
    assert np.abs(flat - src[:1]).max() <= 1e-9 * np.abs(src).max()


def test_outside_voxels_and_the_float_output():
    src = (np.random.default_rng(3).standard_normal((4, 5, 6)) * 1000).astype(np.float32)
    sp, o = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    geom = (sp, o, (6, 7, 8), sp, (-1.0, -1.0, -1.0))
    a = B.resample(src, *geom, order=3, default=-7.5)
    b = B.resample(src, *geom, order=3, extrapolate=True, default=-7.5)
    assert a.dtype == b.dtype == np.float32
    assert (a[0] == -7.5).all() and (a[:, 0] == -7.5).all() and (a[:, :, 0] == -7.5).all()
    assert np.array_equal(b[0, 0, 1:7], src[0, 0]) and b[0, 0, 0] == src[0, 0, 0] and b[5, 6, 7] == src[3, 4, 5]
    assert np.array_equal(a[1:5, 1:6, 1:7], b[1:5, 1:6, 1:7])


def test_window():
    v = np.array([-1e9, -500.0, np.nextafter(-500.0, -np.inf), np.nextafter(-500.0, 0), 0.0, 250.0, 1000.0,
                  999.0, np.nextafter(1000.0, np.inf), np.nan, np.inf, -np.inf])
    got = B.window_u8(v, -500.0, 1000.0)
    assert got.tolist() == [0, 0, 0, 0, 85, 127, 255, 254, 255, 0, 255, 0]
    m = np.array([1.0, 0.0] * 6)
    assert B.window_u8(v, -500.0, 1000.0, mask=m, out_min=3, out_max=200).tolist()[::2] == \
        B.window_u8(v, -500.0, 1000.0, out_min=3, out_max=200).tolist()[::2]
    assert (B.window_u8(v, -500.0, 1000.0, mask=m, out_min=3)[1::2] == 0).all()
