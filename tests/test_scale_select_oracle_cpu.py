"""CPU test of tests/scale_select_oracle.py, the checker of ife_scale_select: on features of the
CPU oracle it finds a Gaussian blob and a Gaussian-profile tube at the scale theory says, and it
keeps the rules of the fold (the first of equal scales, no NaN, zero features give (0, 255))."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scale_select_oracle as Q  # noqa: E402

N = 33
SIGMAS = [1.0, 1.5, 2.0, 3.0, 4.0]
CENTRE = (N // 2, N // 2, N // 2)


@pytest.fixture(scope="module")
def shapes(oracle):
    """The features [S][33][33][33][8] of a Gaussian blob of width 2.45 and of a tube of width 2
    along z, amplitude 100, no mask."""
    z, y, x = np.meshgrid(*(np.arange(N, dtype=np.float64) - N // 2,) * 3, indexing="ij")
    blob = (100.0 * np.exp(-(x * x + y * y + z * z) / (2 * 2.45 ** 2))).astype(np.float32)
    tube = (100.0 * np.exp(-(x * x + y * y) / (2 * 2.0 ** 2))).astype(np.float32)
    ones = np.ones((N, N, N), np.uint8)
    feats = {name: np.stack([oracle.emphysema_features(img, ones, s) for s in SIGMAS])
             for name, img in (("blob", blob), ("tube", tube))}
    return feats


def test_blob_and_tube_peak_at_the_third_scale(shapes):
    lap = Q.measure(Q.LAPLACIAN, 1, 1.0)
    tube = Q.measure(Q.TUBE, 1, 1.0, 0.5, 0.5, 15.0)
    # the normalised -LoG at the centre rises to sigma = 2 and falls behind it
    for name, want in (("blob", [33.1, 49.7, 54.9, 45.2, 31.0]), ("tube", [30.6, 44.6, 48.8, 42.0, 31.8])):
        R = Q.responses(shapes[name], SIGMAS, lap)[(slice(None),) + CENTRE]
        assert R.dtype == np.float32
        assert np.allclose(R, want, atol=0.06), (name, R)
        resp, idx = Q.scale_select(shapes[name], SIGMAS, [lap])
        assert idx[0][CENTRE] == 2 and resp[0][CENTRE] == R[2]
    resp, idx = Q.scale_select(shapes["tube"], SIGMAS, [tube])
    assert idx[0][CENTRE] == 2 and 0 < resp[0][CENTRE] <= 1
    # a blob is no tube: its three curvatures are equal, so 1 - A is small beside the tube's
    blob_as_tube = Q.scale_select(shapes["blob"], SIGMAS, [tube])[0][0][CENTRE]
    assert blob_as_tube < 0.5 * resp[0][CENTRE]


def test_the_other_polarity_finds_nothing_there(shapes):
    for name in ("blob", "tube"):
        resp, idx = Q.scale_select(shapes[name], SIGMAS, [Q.measure(Q.LAPLACIAN, -1, 1.0),
                                                          Q.measure(Q.TUBE, -1, 1.0, 0.5, 0.5, 15.0)])
        assert (resp[:, CENTRE[0], CENTRE[1], CENTRE[2]] == 0).all()
        assert (idx[:, CENTRE[0], CENTRE[1], CENTRE[2]] == Q.NONE).all()


def _features(rows):
    """[S][n][8] from rows of (e1, e2, e3, L) per scale."""
    f = np.zeros((len(rows), len(rows[0]), 8), np.float32)
    f[..., 2:6] = np.asarray(rows, np.float32)
    return f


def test_ties_take_the_first_scale():
    f = _features([[(-1, 0, 0, -3)], [(-1, 0, 0, -3)], [(-1, 0, 0, -2)]])
    resp, idx = Q.scale_select(f, [2.0, 2.0, 2.0], [Q.measure(Q.LAPLACIAN, 1, 0.0)])
    assert resp[0][0] == 3 and idx[0][0] == 0
    # a repeated sigma never wins over its first occurrence, whatever the measure
    f = _features([[(-4, -3, -1, -8)], [(-5, -3, -1, -9)], [(-4, -3, -1, -8)], [(-5, -3, -1, -9)]])
    ms = [Q.measure(k, 1, 1.0, 0.5, 0.5, 3.0) for k in (Q.LAPLACIAN, Q.TUBE, Q.PLATE, Q.BLOB)]
    resp, idx = Q.scale_select(f, [1.0, 1.5, 1.0, 1.5], ms)
    assert (idx <= 1).all() and (resp > 0).all()


def test_nan_features_never_win():
    nan = np.nan
    f = _features([[(-2, -1, -1, -4)], [(nan, nan, nan, nan)], [(-2, nan, -1, nan)]])
    ms = [Q.measure(k, 1, 0.0, 0.5, 0.5, 1.0) for k in (Q.LAPLACIAN, Q.TUBE, Q.PLATE, Q.BLOB)]
    resp, idx = Q.scale_select(f, [1.0, 2.0, 3.0], ms)
    assert np.isfinite(resp).all() and (idx == 0).all() and (resp > 0).all()
    resp, idx = Q.scale_select(f[1:], [2.0, 3.0], ms)        # NaN alone: nothing
    assert (resp == 0).all() and (idx == Q.NONE).all()


def test_plate_with_a_zero_middle_eigenvalue_is_c():
    f = _features([[(-3, 0, 0, -3)]])
    m = Q.measure(Q.PLATE, 1, 1.0, 0.5, 0.5, 4.0)
    R = Q.responses(f, [2.0], m)
    a3 = 4.0 * 3.0
    assert R[0][0] == 1.0 - np.exp(-(a3 * a3) * float(Q.reciprocal(4.0)))      # A = B = 1
    # and the tube and the blob need a2 to have the sign
    for kind in (Q.TUBE, Q.BLOB):
        assert Q.responses(f, [2.0], Q.measure(kind, 1, 1.0, 0.5, 0.5, 4.0))[0][0] == 0


def test_zero_features_give_nothing():
    f = np.zeros((3, 5, 8), np.float32)
    ms = [Q.measure(k, p, 1.0, 0.5, 0.5, 1.0) for k in (Q.LAPLACIAN, Q.TUBE, Q.PLATE, Q.BLOB) for p in (1, -1)]
    resp, idx = Q.scale_select(f, [1.0, 2.0, 3.0], ms)
    assert resp.dtype == np.float32 and idx.dtype == np.uint8
    assert (resp == 0).all() and not np.signbit(resp).any() and (idx == Q.NONE).all()


def test_signs_decide_which_kind_answers():
    """Bright: negative curvature.  (-, -, +) in e1, e2, e3 is a tube and a plate, no blob."""
    f = _features([[(-5, -4, 1, -8), (5, 4, 1, 10), (-5, 4, -1, -2)]])
    got = {k: Q.responses(f, [1.0], Q.measure(k, 1, 1.0, 0.5, 0.5, 3.0))[0] for k in (Q.TUBE, Q.PLATE, Q.BLOB)}
    assert got[Q.TUBE][0] > 0 and got[Q.PLATE][0] > 0 and got[Q.BLOB][0] == 0
    assert got[Q.TUBE][1] == got[Q.PLATE][1] == got[Q.BLOB][1] == 0
    assert got[Q.TUBE][2] == 0 and got[Q.PLATE][2] > 0 and got[Q.BLOB][2] == 0
    dark = {k: Q.responses(f, [1.0], Q.measure(k, -1, 1.0, 0.5, 0.5, 3.0))[0] for k in (Q.TUBE, Q.PLATE, Q.BLOB)}
    assert dark[Q.TUBE][1] > 0 and dark[Q.PLATE][1] > 0 and dark[Q.BLOB][1] > 0
    assert dark[Q.TUBE][0] == dark[Q.PLATE][0] == dark[Q.BLOB][0] == 0
