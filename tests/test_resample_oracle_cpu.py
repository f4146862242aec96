"""tests/resample_oracle.py held to facts that do not depend on it: a linear ramp on dyadic
geometry is reproduced exactly, the half-voxel border band carries the edge voxel, a dyadic
identity returns the source bit for bit (infinities and NaNs included), nearest takes the upper
voxel on exact halves, and the nearest index of a one-voxel axis stays 0."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_oracle as R  # noqa: E402


def _ramp(shape, spacing, origin):
    """3x - 2y + 5z + 1 at the physical points of a grid (dyadic geometry: exact)."""
    z, y, x = np.meshgrid(*(origin[2 - a] + np.arange(shape[a]) * spacing[2 - a] for a in range(3)),
                          indexing="ij")
    return 3 * x - 2 * y + 5 * z + 1


SRC_SHAPE, SRC_SPACING, SRC_ORIGIN = (6, 7, 9), (0.5, 0.25, 2.0), (-3.0, 1.5, 0.25)
DST_SHAPE, DST_SPACING, DST_ORIGIN = (40, 20, 45), (0.125, 0.125, 0.375), (-3.5, 1.25, -1.0)


def _c(axis):
    """continuous source index of every output index along an axis (0 = x), exact here"""
    n = DST_SHAPE[2 - axis]
    return (DST_ORIGIN[axis] + np.arange(n) * DST_SPACING[axis] - SRC_ORIGIN[axis]) / SRC_SPACING[axis]


def test_ramp_is_reproduced_and_border_band_holds_the_edge_voxel():
    src = _ramp(SRC_SHAPE, SRC_SPACING, SRC_ORIGIN)
    got = R.resample(src, SRC_SPACING, SRC_ORIGIN, DST_SHAPE, DST_SPACING, DST_ORIGIN, default=-7.5)
    cx, cy, cz = _c(0), _c(1), _c(2)
    ns = {0: SRC_SHAPE[2], 1: SRC_SHAPE[1], 2: SRC_SHAPE[0]}
    ins = [(c >= -0.5) & (c < ns[a] - 0.5) for a, c in enumerate((cx, cy, cz))]
    core = [(c >= 0) & (c <= ns[a] - 1) for a, c in enumerate((cx, cy, cz))]
    inside = ins[2][:, None, None] & ins[1][None, :, None] & ins[0][None, None, :]
    interior = core[2][:, None, None] & core[1][None, :, None] & core[0][None, None, :]
    assert 0 < interior.sum() < inside.sum() < inside.size
    want = _ramp(DST_SHAPE, DST_SPACING, DST_ORIGIN)
    assert np.array_equal(got[interior], want[interior])
    assert (got[~inside] == -7.5).all()
    # the band: the value of the source voxel with every index clamped to the grid
    clamped = [np.clip(c, 0, ns[a] - 1) for a, c in enumerate((cx, cy, cz))]
    z, y, x = np.meshgrid(*(SRC_ORIGIN[a] + clamped[a] * SRC_SPACING[a] for a in (2, 1, 0)), indexing="ij")
    edge = 3 * x - 2 * y + 5 * z + 1
    band = inside & ~interior
    assert band.any() and np.array_equal(got[band], edge[band])


def test_dyadic_identity_returns_the_source_with_inf_and_nan():
    rng = np.random.default_rng(5)
    shape, spacing, origin = (5, 6, 7), (0.75, 0.75, 0.75), (-3.25, -3.25, -3.25)
    src = rng.standard_normal(shape)
    src[1, 2, 3], src[0, 0, 0], src[4, 5, 6] = np.inf, -np.inf, np.nan
    src[2, 2, 2] = np.array([0x7ff8000000abcdef], np.uint64).view(np.float64)[0]   # a NaN with a payload
    for interp in (R.LINEAR, R.NEAREST):
        got = R.resample(src, spacing, origin, shape, spacing, origin, interpolation=interp, default=-1.0)
        assert np.array_equal(R.bits(got), R.bits(src))
    s32 = src.astype(np.float32)
    got = R.resample(s32, spacing, origin, shape, spacing, origin)
    assert got.dtype == np.float32 and np.array_equal(R.bits(got), R.bits(s32))


def test_nearest_takes_the_upper_voxel_on_exact_halves():
    src = np.arange(8, dtype=np.uint16).reshape(1, 1, 8) * 10
    # 2:1 refinement from the same origin: c = i / 2
    got = R.resample(src, (1.0, 1.0, 1.0), (0, 0, 0), (1, 1, 16), (0.5, 1.0, 1.0), (0, 0, 0),
                     interpolation=R.NEAREST, default=999)
    c = np.arange(16) / 2
    inside = c < 7.5
    want = np.where(inside, 10 * np.minimum(np.floor(c + 0.5), 7), 999).astype(np.uint16)
    assert got.dtype == np.uint16 and np.array_equal(got[0, 0], want)
    assert got[0, 0, 1] == 10 and got[0, 0, 3] == 20 and got[0, 0, 15] == 999   # c = 0.5 -> 1, 1.5 -> 2


def test_one_voxel_axis_just_below_a_half_yields_index_zero():
    c = np.nextafter(0.5, 0)
    assert c + 0.5 == 1.0                                   # the rounding that the min is there for
    inside, b, t, skip, near = R.axis_table(1, 1, 1.0, 0.0, 1.0, c, 0.0)
    assert inside[0] and b[0] == 0 and near[0] == 0 and skip[0] and t[0] == c
    src = np.array([[[3.5]]])
    assert R.resample(src, (1, 1, 1), (0, 0, 0), (1, 1, 1), (1, 1, 1), (c, 0, 0), interpolation=R.NEAREST)[0, 0, 0] == 3.5
    assert R.resample(src, (1, 1, 1), (0, 0, 0), (1, 1, 1), (1, 1, 1), (c, 0, 0))[0, 0, 0] == 3.5


def test_huge_translation_is_outside_not_an_error():
    src = np.ones((2, 2, 2))
    for tr in ((1e300, 0, 0), (0, 0, -1e300)):
        got = R.resample(src, (1, 1, 1), (0, 0, 0), (2, 2, 2), (1, 1, 1), (0, 0, 0), tr, default=4.0)
        assert (got == 4.0).all()
