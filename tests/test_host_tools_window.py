"""The ExtractWindow tool (host/tools/ExtractWindow.cxx: the reference's -i -o -m -w -l -b, and our
-S) and the -b flag of Resample.  Without a GPU: the flags, the usage and the refusal of an order
above 5.  On the device: the tool's output file equals, byte for byte, the oracle's composition
(tests/bspline_oracle.py: B-spline resampling with nearest extrapolation, the window, the mask at
order 0) on the grid the tool forms; `Resample -b 3` equals Context.resample_bspline, and Resample
without -b is what it was."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "image-feature-extraction_amd", "host", "bin")
EXTRACT, RESAMPLE = os.path.join(BIN, "ExtractWindow"), os.path.join(BIN, "Resample")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bspline_oracle as B  # noqa: E402
import niftiio  # noqa: E402
import resample_oracle as R  # noqa: E402

# a 9 x 7 x 1 image; the file holds spacings and origins as floats
SHAPE = (1, 7, 9)
SPACING = tuple(float(np.float32(v)) for v in (0.7, 0.6, 1.0))
ORIGIN = (-3.25, 4.5, 0.0)


def test_usage_names_every_flag():
    r = subprocess.run([EXTRACT, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("-i", "--image", "-o", "--out", "-m", "--mask", "-w", "--width", "-l", "--level", "-b",
                 "--spline-order", "-S", "--spacing"):
        assert flag in r.stdout, flag
    r = subprocess.run([RESAMPLE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--spline-order" in r.stdout and "--source" in r.stdout


def test_required_flags_and_the_order_above_five(tmp_path):
    r = subprocess.run([EXTRACT, "-o", str(tmp_path / "o.nii")], capture_output=True, text=True)
    assert r.returncode != 0
    for tool, args in ((EXTRACT, ["-i", "absent.nii", "-o", str(tmp_path / "o.nii")]),
                       (RESAMPLE, ["-s", "absent.nii", "-t", "absent.nii", "-o", str(tmp_path / "o.nii")])):
        r = subprocess.run([tool] + args + ["-b", "6"], capture_output=True, text=True)
        assert r.returncode != 0 and "Spline order must be <= 5" in r.stderr
    r = subprocess.run([EXTRACT, "-i", "absent.nii", "-o", str(tmp_path / "o.nii"), "-S", "0"], capture_output=True,
                       text=True)
    assert r.returncode != 0 and "Spacing must be positive" in r.stderr
    assert not os.path.exists(str(tmp_path / "o.nii"))


def _target(shape, spacing, S=0.25):
    """the grid the tool forms: ceil(n * s / S) voxels of S per axis of more than one voxel"""
    size = tuple(n if n < 2 else int(math.ceil((float(n) * s) / S)) for n, s in zip(shape[::-1], spacing))
    return size[::-1], tuple(s if n < 2 else S for n, s in zip(shape[::-1], spacing))


@pytest.mark.gpu
@pytest.mark.parametrize("order", [3, 5, 0])
def test_extract_window_equals_the_oracle_composition(tmp_path, order):
    rng = np.random.default_rng(40 + order)
    image = rng.integers(-1400, 500, SHAPE).astype(np.int16)
    mask = (rng.integers(0, 3, SHAPE) > 0).astype(np.uint8)
    i, m = str(tmp_path / "image.nii"), str(tmp_path / "mask.nii")
    niftiio.write(i, image, SPACING, geometry={"qoffset": ORIGIN})
    niftiio.write(m, mask, SPACING, geometry={"qoffset": ORIGIN})
    d_shape, d_spacing = _target(SHAPE, SPACING)
    assert d_shape == (1, 17, 26) and d_spacing == (0.25, 0.25, 1.0)
    geom = (SPACING, ORIGIN, d_shape, d_spacing, (0.0, 0.0, 0.0), ORIGIN)
    fine = B.resample(image.astype(np.float64), *geom, order=order, extrapolate=True)
    fine_mask = B.resample(mask.astype(np.float64), *geom, order=0, extrapolate=True)
    assert set(np.unique(fine_mask)) == {0.0, 1.0}
    for with_mask in (False, True):
        o = str(tmp_path / ("out%d.nii" % with_mask))
        r = subprocess.run([EXTRACT, "-i", i, "-o", o, "-b", str(order)] + (["-m", m] if with_mask else []),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got, spacing = niftiio.read(o)
        want = B.window_u8(fine, -500.0 - 750.0, -500.0 + 750.0, mask=fine_mask if with_mask else None)
        assert got.dtype == np.uint8 and got.shape == d_shape
        assert got.tobytes() == want.tobytes()
        assert spacing[:2] == (0.25, 0.25) and niftiio.read_geometry(o)["qoffset"] == (0.0, 0.0, 0.0)
        assert "Resampling image." in r.stderr and ("Resampling mask." in r.stderr) == with_mask
        assert 0 < (want == 0).mean() < 1 and 0 < (want == 255).mean() < 1 and ((want > 0) & (want < 255)).any()
    # a narrower window and a coarser grid through the flags
    o = str(tmp_path / "out_flags.nii")
    r = subprocess.run([EXTRACT, "-i", i, "-o", o, "-b", str(order), "-w", "400", "-l", "40", "-S", "0.5"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d_shape, d_spacing = _target(SHAPE, SPACING, 0.5)
    fine = B.resample(image.astype(np.float64), SPACING, ORIGIN, d_shape, d_spacing, (0.0, 0.0, 0.0), ORIGIN,
                      order=order, extrapolate=True)
    assert niftiio.read(o)[0].tobytes() == B.window_u8(fine, 40.0 - 200.0, 40.0 + 200.0).tobytes()


SRC_SHAPE, SRC_SPACING, SRC_ORIGIN = (9, 20, 24), (0.75, 0.75, 2.5), (-120.5, 37.25, 0.0)
DST_SHAPE, DST_SPACING, DST_ORIGIN = (36, 20, 24), (0.75, 0.75, 0.625), (37.25, -120.5, 8.0)
T = tuple(a - b for a, b in zip(SRC_ORIGIN, DST_ORIGIN))


def _resample_tool(tmp_path, src, extra):
    s, t, o = (str(tmp_path / n) for n in ("source.nii.gz", "target.nii.gz", "out.nii.gz"))
    niftiio.write(s, src, SRC_SPACING, geometry={"qoffset": SRC_ORIGIN})
    niftiio.write(t, np.zeros(DST_SHAPE, np.uint8), DST_SPACING, geometry={"qoffset": DST_ORIGIN})
    r = subprocess.run([RESAMPLE, "-s", s, "-t", t, "-o", o] + extra, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    vol, spacing = niftiio.read(o)
    assert vol.dtype == np.float64 and vol.shape == DST_SHAPE and spacing == DST_SPACING
    assert niftiio.read_geometry(o)["qoffset"] == DST_ORIGIN
    return r, vol


@pytest.mark.gpu
def test_resample_with_a_spline_order_equals_the_context(tmp_path, ctx):
    src = np.random.default_rng(41).integers(-1000, 1000, SRC_SHAPE, dtype=np.int16)
    r, got = _resample_tool(tmp_path, src, ["-b", "3"])
    want = ctx.resample_bspline(src.astype(np.float64), SRC_SPACING, SRC_ORIGIN, DST_SHAPE, DST_SPACING, DST_ORIGIN,
                                translation=T, order=3)
    assert np.array_equal(B.bits(got), B.bits(want))
    assert np.array_equal(B.bits(got), B.bits(B.resample(src.astype(np.float64), SRC_SPACING, SRC_ORIGIN, DST_SHAPE,
                                                         DST_SPACING, DST_ORIGIN, T, 3)))
    assert "Translation: [-157.75, 157.75, -8]" in r.stdout.splitlines() and (got[34:] == 0).all()
    linear = R.resample(src.astype(np.float64), SRC_SPACING, SRC_ORIGIN, DST_SHAPE, DST_SPACING, DST_ORIGIN, T)
    assert not np.array_equal(got, linear)


@pytest.mark.gpu
def test_resample_without_the_flag_is_unchanged(tmp_path):
    src = np.random.default_rng(42).integers(-1000, 1000, SRC_SHAPE, dtype=np.int16)
    r, got = _resample_tool(tmp_path, src, [])
    want = R.resample(src.astype(np.float64), SRC_SPACING, SRC_ORIGIN, DST_SHAPE, DST_SPACING, DST_ORIGIN, T)
    assert np.array_equal(R.bits(got), R.bits(want))
    lines = r.stdout.splitlines()
    assert lines[0] == "== Source ==" and "Translation: [-157.75, 157.75, -8]" in lines
    assert "Source image information after resampling" in lines
