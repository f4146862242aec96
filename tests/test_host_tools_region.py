"""The four preprocessing tools (ExtractBoundingBox, ExtractMaskedRegion, ExtractSlices, PadImage):
the reference's flags and messages without a device, and on the device outputs that are byte-equal
to tests/region_oracle.py's from small NIfTI files."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "image-feature-extraction_amd", "host")
BIN = os.path.join(HOST, "bin")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niftiio  # noqa: E402
import region_oracle as R  # noqa: E402

FLAGS = {
    "ExtractBoundingBox": ["-i", "--image", "-m", "--mask", "-o", "--out"],
    "ExtractMaskedRegion": ["-m", "--mask", "-o", "--out", "-i", "--include", "-I", "--inside", "-O", "--outside"],
    "ExtractSlices": ["-i", "--image", "-o", "--out", "-t", "--type", "-m", "--mask", "-s", "--slice-index", "-l",
                      "--slice-location", "-w", "--slice-window", "-d", "--slice-stride", "-a", "--axis-index"],
    "PadImage": ["-i", "--image", "-o", "--out", "-x", "--size-x", "-y", "--size-y", "-p", "--pad-value"],
}


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "image-feature-extraction_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return {name: os.path.join(BIN, name) for name in FLAGS}


def run(tool, *args):
    return subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True)


# ---- without a GPU: the checks that come before any image is read -------------------------------
@pytest.mark.parametrize("name", sorted(FLAGS))
def test_help_names_every_flag(tools, name):
    r = run(tools[name], "--help")
    assert r.returncode == 0
    for flag in FLAGS[name]:
        assert flag + "," in r.stdout or flag + " " in r.stdout, flag


@pytest.mark.parametrize("name,args", [
    ("ExtractBoundingBox", ["-i", "none.nii", "-o", "out.nii"]),              # -m
    ("ExtractMaskedRegion", ["-m", "none.nii", "-o", "out.nii"]),             # -i is required
    ("ExtractSlices", ["-i", "none.nii"]),                                    # -o
    ("PadImage", ["-i", "none.nii", "-o", "out.nii", "-x", "4"]),             # -y
])
def test_a_missing_required_flag(tools, tmp_path, name, args):
    r = subprocess.run([tools[name]] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "Required argument missing" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_slices_axis_out_of_range(tools, tmp_path):
    r = run(tools["ExtractSlices"], "-i", tmp_path / "none.nii", "-o", tmp_path / "s_", "-a", 3)
    assert r.returncode != 0 and "Axis index must be less than the number of dimensions" in r.stderr


def test_slices_window_without_stride_is_refused(tools, tmp_path):
    """The reference loops forever here (its offset never advances); ours says so and stops."""
    r = run(tools["ExtractSlices"], "-i", tmp_path / "none.nii", "-o", tmp_path / "s_", "-s", 3, "-w", 4, "-d", 0)
    assert r.returncode != 0 and "Slice stride must be positive" in r.stderr
    r = run(tools["ExtractSlices"], "-i", tmp_path / "none.nii", "-o", tmp_path / "s_", "-s", 3, "-w", 4)
    assert r.returncode != 0 and "Slice stride must be positive" in r.stderr
    r = run(tools["ExtractSlices"], "-i", tmp_path / "none.nii", "-o", tmp_path / "s_", "-t", "png")
    assert r.returncode != 0 and "suffix" in r.stderr


# ---- on the device ------------------------------------------------------------------------------
SHAPE = (9, 11, 70)
SPACING = (0.7, 0.8, 2.5)


def image(dtype):
    rng = np.random.default_rng(61)
    if np.issubdtype(dtype, np.integer):
        return rng.integers(-2000, 2000, SHAPE).astype(dtype)
    return rng.normal(-500, 300, SHAPE).astype(dtype)


def box_mask():
    m = np.zeros(SHAPE, np.uint8)
    m[2:7, 3:9, 17:50] = 1
    m[4, 5, 11] = 3        # clamped to 1; widens the box in x
    m[7, 2, 30] = 255
    return m


def rotated_geometry():
    c, s = np.cos(0.4), np.sin(0.4)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    srow = np.hstack([rot @ np.diag(SPACING), [[-101.3], [57.7], [-300.1]]]).astype(np.float32)
    # the quaternion of a rotation by 0.4 about z
    return {"qform_code": (1,), "sform_code": (2,), "quatern": (0.0, 0.0, float(np.sin(0.2))),
            "qoffset": (-101.3, 57.7, -300.1), "srow_x": tuple(srow[0]), "srow_y": tuple(srow[1]),
            "srow_z": tuple(srow[2]), "qfac": (1.0,)}, srow


@pytest.mark.gpu
def test_bounding_box_crop_and_its_geometry(tools, tmp_path):
    img, mask = image(np.float32), box_mask()
    geom, srow = rotated_geometry()
    ip, mp, op = str(tmp_path / "img.nii"), str(tmp_path / "mask.nii.gz"), str(tmp_path / "out.nii")
    niftiio.write(ip, img, SPACING, geometry=geom)
    niftiio.write(mp, mask, SPACING)
    r = run(tools["ExtractBoundingBox"], "-i", ip, "-m", mp, "-o", op)
    assert r.returncode == 0, r.stderr
    index, size, count = R.bounding_box(mask)
    assert index == (11, 2, 2) and size == (39, 7, 6)
    got, spacing = niftiio.read(op)
    assert got.tobytes() == R.extract_region(img, index, size).tobytes() and got.shape == size[::-1]
    assert spacing == tuple(np.float32(SPACING))
    g = niftiio.read_geometry(op)
    assert g["qform_code"] == (1,) and g["sform_code"] == (2,) and g["quatern"] == niftiio.read_geometry(ip)["quatern"]
    for r_, key in enumerate(("srow_x", "srow_y", "srow_z")):
        assert g[key][:3] == tuple(srow[r_, :3])
    assert R.within_one_ulp([g[k][3] for k in ("srow_x", "srow_y", "srow_z")], R.shift_srow(srow, index))
    want_q = R.shift_qoffset(geom["quatern"], 1.0, np.float32(SPACING).astype(np.float64),
                             np.float32(geom["qoffset"]), index)
    assert R.within_one_ulp(g["qoffset"], want_q)
    # the two descriptions of the same rotation agree on where the box lies
    assert np.allclose(g["qoffset"], [g[k][3] for k in ("srow_x", "srow_y", "srow_z")], atol=1e-3)


@pytest.mark.gpu
def test_bounding_box_of_an_empty_mask_and_of_a_larger_mask(tools, tmp_path):
    ip, mp, op = str(tmp_path / "img.nii"), str(tmp_path / "mask.nii"), str(tmp_path / "out.nii")
    niftiio.write(ip, image(np.float32), SPACING)
    niftiio.write(mp, np.zeros(SHAPE, np.uint8), SPACING)
    r = run(tools["ExtractBoundingBox"], "-i", ip, "-m", mp, "-o", op)
    assert r.returncode != 0 and "Error calculating bounding box." in r.stderr and not os.path.exists(op)
    big = np.zeros((SHAPE[0], SHAPE[1], SHAPE[2] + 4), np.uint8)
    big[1:3, 1:3, 60:] = 1   # the box reaches beyond the image
    niftiio.write(mp, big, SPACING)
    r = run(tools["ExtractBoundingBox"], "-i", ip, "-m", mp, "-o", op)
    assert r.returncode != 0 and "Failed to write image." in r.stderr and not os.path.exists(op)
    assert "Bounding box:    ImageRegion Index: [60, 1, 1] Size: [14, 2, 2]" in r.stderr


@pytest.mark.gpu
def test_masked_region(tools, tmp_path):
    rng = np.random.default_rng(62)
    lab = rng.choice(np.array([0, 1, 3, 255, 256, 900, 65535], np.uint16), SHAPE)
    mp, op = str(tmp_path / "lab.nii"), str(tmp_path / "out.nii.gz")
    niftiio.write(mp, lab, SPACING)
    r = run(tools["ExtractMaskedRegion"], "-m", mp, "-o", op, "-i", 900, "-i", 3, "-i", 256, "-i", 3)
    assert r.returncode == 0, r.stderr
    got, spacing = niftiio.read(op)
    assert got.dtype == np.uint16 and got.tobytes() == R.label_membership(lab, [3, 256, 900]).tobytes()
    assert spacing == tuple(np.float32(SPACING))
    r = run(tools["ExtractMaskedRegion"], "-m", mp, "-o", op, "-i", 65535, "-I", 65535, "-O", 7)
    assert r.returncode == 0, r.stderr
    assert niftiio.read(op)[0].tobytes() == R.label_membership(lab, [65535], 65535, 7).tobytes()


def slice_indices(n, given, locations, window, stride):
    """The index set of the reference's tools/ExtractSlices.cxx:166-212, restated: locations
    become indices through round(location * (n - 1)); neighbours at multiples of the stride up to
    half the window, kept where they stay inside; sorted, unique."""
    idx = list(given)
    for loc in locations:
        if 0 <= loc <= 1:
            idx.append(int(np.floor(loc * (n - 1) + 0.5)))
    if not idx:
        return list(range(n))
    for i in list(idx):
        off = stride
        while window // 2 > 0 and off <= window // 2:
            if i - off >= 0:
                idx.append(i - off)
            if i + off < n:
                idx.append(i + off)
            off += stride
    return sorted(set(idx))


def expected_slice(vol, box_index, box_size, axis, k):
    """(z = 1, b, a) of the two remaining axes in order, flipped along the volume's z for axes 0, 1"""
    (x0, y0, z0), (sx, sy, sz) = box_index, box_size
    sub = vol[z0:z0 + sz, y0:y0 + sy, x0:x0 + sx]
    if axis == 2:
        return sub[k][None]
    plane = sub[:, k, :] if axis == 1 else sub[:, :, k]
    return np.ascontiguousarray(plane[::-1])[None]


SLICE_CASES = [
    # axis, mask, extra arguments, (given, locations, window, stride)
    (2, False, [], ((), (), 0, 0)),
    (1, False, ["-s", 0, "-s", 10, "-s", 4], ((0, 10, 4), (), 0, 0)),
    (0, False, ["-l", 0.0, "-l", 0.5, "-l", 1.0, "-l", 1.5], ((), (0.0, 0.5, 1.0), 0, 0)),
    (2, True, [], ((), (), 0, 0)),
    (1, True, ["-l", 0.5, "-w", 5, "-d", 2], ((), (0.5,), 5, 2)),
    (0, True, ["-s", 1, "-s", 37, "-w", 6, "-d", 1], ((1, 37), (), 6, 1)),
    (2, True, ["-s", 2, "-w", 20, "-d", 3], ((2,), (), 20, 3)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("axis,with_mask,extra,rule", SLICE_CASES)
def test_slices(tools, tmp_path, axis, with_mask, extra, rule):
    vol, mask = image(np.float64), box_mask()
    ip, mp, base = str(tmp_path / "img.nii"), str(tmp_path / "mask.nii"), str(tmp_path / "s_")
    niftiio.write(ip, vol, SPACING, geometry=rotated_geometry()[0])
    niftiio.write(mp, mask, SPACING)
    args = ["-i", ip, "-o", base, "-t", "nii", "-a", axis] + (["-m", mp] if with_mask else []) + extra
    r = run(tools["ExtractSlices"], *args)
    assert r.returncode == 0, r.stderr
    index, size = R.bounding_box(mask)[:2] if with_mask else ((0, 0, 0), SHAPE[::-1])
    assert r.stdout.count("Region ImageRegion Index:") == (2 if with_mask else 1)
    assert "Region ImageRegion Index: [%d, %d, %d] Size: [%d, %d, %d]" % (index + size) in r.stdout
    want = slice_indices(size[axis], *rule)
    names = sorted(os.path.basename(p) for p in glob.glob(base + "*"))
    assert names == sorted("s_axis-%d_absslice-%d_relslice-%d.nii" % (axis, index[axis] + k, k) for k in want)
    rest = [a for a in range(3) if a != axis]
    for k in want:
        path = base + "axis-%d_absslice-%d_relslice-%d.nii" % (axis, index[axis] + k, k)
        got, spacing = niftiio.read(path)
        assert got.dtype == np.float64 and got.tobytes() == expected_slice(vol, index, size, axis, k).tobytes(), k
        assert got.shape == (1, size[rest[1]], size[rest[0]])
        assert spacing == (np.float32(SPACING[rest[0]]), np.float32(SPACING[rest[1]]), 1.0)
        g = niftiio.read_geometry(path)   # the file geometry is dropped: identity directions
        assert g["quatern"] == (0.0, 0.0, 0.0) and g["srow_x"][1:3] == (0.0, 0.0)


@pytest.mark.gpu
def test_slices_outside_bounds_and_default_suffix(tools, tmp_path):
    ip, base = str(tmp_path / "img.nii"), str(tmp_path / "s_")
    vol = image(np.float64)
    niftiio.write(ip, vol, SPACING)
    r = run(tools["ExtractSlices"], "-i", ip, "-o", base, "-s", 9)
    assert r.returncode != 0 and "Slice indices are outside bounds" in r.stderr
    assert "Largest requested index is 9" in r.stderr and "Largest possible index is 9" in r.stderr
    assert glob.glob(base + "*") == []
    r = run(tools["ExtractSlices"], "-i", ip, "-o", base, "-s", 8)
    assert r.returncode == 0, r.stderr
    assert [os.path.basename(p) for p in glob.glob(base + "*")] == ["s_axis-2_absslice-8_relslice-8.nii.gz"]
    assert niftiio.read(glob.glob(base + "*")[0])[0].tobytes() == vol[8][None].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,target", [((1, 11, 70), (75, 16)), ((1, 11, 70), (76, 17)), ((3, 11, 70), (70, 12))])
def test_pad(tools, tmp_path, shape, target):
    rng = np.random.default_rng(63)
    img = rng.integers(-2000, 2000, shape).astype(np.int16)
    ip, op = str(tmp_path / "img.nii"), str(tmp_path / "out.nii")
    niftiio.write(ip, img, SPACING, geometry={"qoffset": (10.0, 20.0, 30.0), "qform_code": (1,)})
    r = run(tools["PadImage"], "-i", ip, "-o", op, "-x", target[0], "-y", target[1], "-p", -1000)
    assert r.returncode == 0, r.stderr
    lower = [(t - n) // 2 for t, n in zip(target, (shape[2], shape[1]))]
    upper = [l + (t - n) % 2 for l, t, n in zip(lower, target, (shape[2], shape[1]))]
    want = np.pad(img, ((0, 0), (lower[1], upper[1]), (lower[0], upper[0])), constant_values=-1000)
    got, spacing = niftiio.read(op)
    assert want.shape == (shape[0], target[1], target[0]) and got.shape == want.shape
    assert got.dtype == np.int16 and got.tobytes() == want.tobytes()
    assert got.tobytes() == R.extract_region(img, (-lower[0], -lower[1], 0), (target[0], target[1], shape[0]),
                                             -1000).tobytes()
    q = niftiio.read_geometry(op)["qoffset"]   # identity quaternion: the origin moves by -lower o spacing
    assert R.within_one_ulp(q, R.shift_qoffset((0, 0, 0), 1.0, np.float32(SPACING).astype(np.float64),
                                               (10.0, 20.0, 30.0), (-lower[0], -lower[1], 0)))


@pytest.mark.gpu
def test_pad_target_too_small(tools, tmp_path):
    ip, op = str(tmp_path / "img.nii"), str(tmp_path / "out.nii")
    niftiio.write(ip, np.zeros((1, 11, 70), np.int16), SPACING)
    r = run(tools["PadImage"], "-i", ip, "-o", op, "-x", 69, "-y", 16)
    assert r.returncode != 0 and "Error padding image." in r.stderr and not os.path.exists(op)
