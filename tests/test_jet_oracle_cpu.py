"""Pins tests/jet_oracle.py, the numpy oracle of the differential normalized convolution, against
what is already pinned (the CPU oracle's normalized convolution and its first-order differential
form) and against a field whose derivatives are known; and checks that library and binding
expose the new entry points.  No GPU."""
import numpy as np
import pytest

import jet_oracle

NEW_NAMES = ("ife_stage_recursive_gaussian_order", "ife_normalized_convolution_jet",
             "ife_differential_features")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_full_certainty_value_is_the_normalized_convolution(oracle):
    shape, spacing, sigma = (12, 14, 16), (0.7, 1.3, 1.0), 1.5
    img = (np.random.default_rng(1).standard_normal(shape) * 100).astype(np.float32)
    ones = np.ones(shape, np.float32)
    got = jet_oracle.jet(oracle, img, ones, sigma, spacing)[..., 0]
    want = oracle.normalized_gaussian_convolution(img, ones, sigma, spacing)
    np.testing.assert_array_equal(_bits(got), _bits(want))


def test_scaling_the_certainty_changes_no_bit(oracle):
    shape, spacing, sigma = (12, 14, 16), (0.7, 1.3, 1.0), 1.5
    rng = np.random.default_rng(2)
    img = (rng.standard_normal(shape) * 100).astype(np.float32)
    cert = (rng.random(shape) < 0.7).astype(np.float32)
    a = jet_oracle.jet(oracle, img, cert, sigma, spacing)
    b = jet_oracle.jet(oracle, img, cert * np.float32(0.5), sigma, spacing)
    np.testing.assert_array_equal(_bits(a), _bits(b))


def test_quadratic_field_has_its_analytic_derivatives(oracle):
    shape, spacing, sigma = (24, 20, 28), (0.7, 1.3, 1.0), 1.5
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    X, Y, Z = x * spacing[0], y * spacing[1], z * spacing[2]
    q = 0.5 * (X * X + 2 * Y * Y - 3 * Z * Z) + 0.25 * X * Y - 0.5 * X * Z + 0.75 * Y * Z + 2 * X - Y + 3
    j = jet_oracle.jet(oracle, q.astype(np.float32), np.ones(shape, np.float32), sigma, spacing)
    blk = (slice(10, 14), slice(8, 12), slice(12, 16))
    hess = np.abs(j[blk][..., 4:] - np.array([1, 0.25, -0.5, 2, 0.75, -3])).max()
    gx, gy, gz = X + 0.25 * Y - 0.5 * Z + 2, 2 * Y + 0.25 * X + 0.75 * Z - 1, -3 * Z - 0.5 * X + 0.75 * Y
    gm = np.sqrt(gx * gx + gy * gy + gz * gz)[blk]
    got = np.sqrt((j[blk][..., 1:4].astype(np.float64) ** 2).sum(-1))
    grad = (np.abs(got - gm) / gm).max()
    print("quadratic: worst Hessian error %.3g, worst relative gradient magnitude error %.3g" % (hess, grad))
    assert hess <= 1e-2
    assert grad <= 1e-3


@pytest.mark.parametrize("shape,sigma", [((24, 20, 28), 2.0), ((5, 7, 9), 0.8), ((12, 70, 67), 2.5)])
def test_first_derivatives_match_the_first_order_form(oracle, shape, sigma):
    """The two differ only in float against double evaluation of the quotient rule."""
    spacing = (0.7, 1.3, 1.0)
    rng = np.random.default_rng(3)
    img = (rng.standard_normal(shape) * 100).astype(np.float32)
    cert = (rng.random(shape) < 0.7).astype(np.float32)
    j = jet_oracle.jet(oracle, img, cert, sigma, spacing)
    for axis in range(3):
        ref = oracle.differential_normalized_convolution(img, cert, sigma, axis, spacing)
        err = np.abs(j[..., 1 + axis].astype(np.float64) - ref).max() / np.abs(ref).max()
        print("shape %s sigma %g axis %d: max abs difference %.3g of max |derivative|" % (shape, sigma, axis, err))
        assert err <= 1e-6


def test_library_and_binding_expose_the_new_entry_points(ife):
    lib = ife.load_library()
    for name in NEW_NAMES:
        assert name in ife.EXPORTS
        assert hasattr(lib, name)
    for method in ("stage_recursive_gaussian_order", "normalized_convolution_jet", "differential_features",
                   "differential_features_device"):
        assert hasattr(ife.Context, method)
