"""The three ROI tools (GenerateROIs, GenerateROIsManyRegions, SampleROIs): the reference's flags
and messages without a device, and on the device files that equal tests/sampling_oracle.py's lines
from small NIfTI files with IFE_SEED=7; MakeBag's generated regions and the sampled branch of the
edges tool under IFE_DEVICE_SAMPLING=1."""
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
import sampling_oracle as S  # noqa: E402

GEN = ["-m", "--mask", "-o", "--outfile", "-n", "--num-rois", "-x", "--roi-size-x", "-y", "--roi-size-y", "-z",
       "--roi-size-z", "-M", "--mask-value"]
FLAGS = {
    "GenerateROIs": GEN,
    "GenerateROIsManyRegions": GEN,
    "SampleROIs": ["-i", "--image", "-r", "--roi-file", "-o", "--out", "-R", "--roi-file-has-header"],
}
SHAPE = (9, 11, 70)
SEED = 7


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "image-feature-extraction_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return {name: os.path.join(BIN, name) for name in list(FLAGS) + ["MakeBag"]}


def run(tool, *args, **env):
    return subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True,
                          env=dict(os.environ, IFE_SEED=str(SEED), **env))


# ---- without a GPU: the checks that come before any image is read -------------------------------
@pytest.mark.parametrize("name", sorted(FLAGS))
def test_help_names_every_flag(tools, name):
    r = run(tools[name], "--help")
    assert r.returncode == 0
    for flag in FLAGS[name]:
        assert flag + "," in r.stdout or flag + " " in r.stdout, flag


def test_help_describes_the_tool(tools):
    assert "Generate 3D ROIs." in run(tools["GenerateROIs"], "--help").stdout
    assert "Sample ROIs from an image." in run(tools["SampleROIs"], "--help").stdout


@pytest.mark.parametrize("name,args", [
    ("GenerateROIs", ["-m", "none.nii"]),                        # -o
    ("GenerateROIs", ["-o", "out.ROIInfo"]),                     # -m
    ("GenerateROIsManyRegions", ["-m", "none.nii", "-M", "1"]),  # -o
    ("SampleROIs", ["-i", "none.nii", "-r", "none.txt"]),        # -o
    ("SampleROIs", ["-o", "out.csv", "-r", "none.txt"]),         # -i
])
def test_a_missing_required_flag(tools, tmp_path, name, args):
    r = subprocess.run([tools[name]] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "Required argument missing" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_sample_rois_reads_the_boxes_before_the_image(tools, tmp_path):
    """The box list is read and compared first, as in the reference: a list of two sizes fails
    with the reference's line on stdout, whatever the image is; an empty list is a read error."""
    (tmp_path / "rois.txt").write_text("header\n[1, 2, 3][5, 4, 3]\n[2, 2, 3][5, 4, 2]\n")
    r = run(tools["SampleROIs"], "-i", tmp_path / "none.nii", "-r", tmp_path / "rois.txt", "-o", tmp_path / "o.csv")
    assert r.returncode != 0
    assert r.stdout.splitlines() == ["Got 2 rois.", "ROI size differ: [5, 4, 3] | [5, 4, 2]"]
    assert not (tmp_path / "o.csv").exists()
    # without -R false the first line is a header: one box is left
    (tmp_path / "one.txt").write_text("[1, 2, 3][5, 4, 3]\n[2, 2, 3][5, 4, 2]\n")
    r = run(tools["SampleROIs"], "-i", tmp_path / "none.nii", "-r", tmp_path / "one.txt", "-o", tmp_path / "o.csv")
    assert r.returncode != 0 and r.stdout.splitlines() == ["Got 1 rois.", "ROI size [5, 4, 2]."]
    (tmp_path / "empty.txt").write_text("header\n")
    r = run(tools["SampleROIs"], "-i", tmp_path / "none.nii", "-r", tmp_path / "empty.txt", "-o", tmp_path / "o.csv")
    assert r.returncode != 0 and "Got 0 rois." in r.stdout and "Error reading ROIs" in r.stderr


# ---- on the device ------------------------------------------------------------------------------
def label_mask():
    rng = np.random.default_rng(71)
    m = rng.integers(0, 4, SHAPE).astype(np.uint8)
    m[:, :, :3] = 0
    return m


@pytest.mark.gpu
def test_generate_rois_equals_the_oracle(tools, tmp_path):
    mask = label_mask()
    mp = str(tmp_path / "mask.nii.gz")
    niftiio.write(mp, mask)
    out = tmp_path / "r.ROIInfo"
    r = run(tools["GenerateROIs"], "-m", mp, "-o", out, "-n", 23, "-x", 9, "-y", 4, "-z", 3, "-M", 2)
    assert r.returncode == 0, r.stderr
    want, _ = S.random_rois(mask, 23, (9, 4, 3), values=(2,), per_value=True, seed=SEED)
    assert out.read_text().splitlines() == S.roi_info_lines(want[0])
    # the defaults: 50 boxes of 53 x 53 x 41 on value 1 do not fit this volume
    r = run(tools["GenerateROIs"], "-m", mp, "-o", tmp_path / "d.ROIInfo")
    assert r.returncode != 0 and "Failed to generate ROIs." in r.stderr and "set 0" in r.stderr
    assert not (tmp_path / "d.ROIInfo").exists()
    r = run(tools["GenerateROIs"], "-m", mp, "-o", tmp_path / "e.ROIInfo", "-x", 1, "-y", 1, "-z", 1)
    assert r.returncode == 0, r.stderr
    want, _ = S.random_rois(mask, 50, (1, 1, 1), values=(1,), per_value=True, seed=SEED)
    assert (tmp_path / "e.ROIInfo").read_text().splitlines() == S.roi_info_lines(want[0])
    # an absent value
    r = run(tools["GenerateROIs"], "-m", mp, "-o", tmp_path / "f.ROIInfo", "-x", 1, "-y", 1, "-z", 1, "-M", 9)
    assert r.returncode != 0 and "Failed to generate ROIs." in r.stderr and not (tmp_path / "f.ROIInfo").exists()


@pytest.mark.gpu
def test_generate_rois_many_regions_equals_the_oracle(tools, tmp_path):
    mask = label_mask()
    mp = str(tmp_path / "mask.nii.gz")
    niftiio.write(mp, mask)
    base = str(tmp_path / "many_")
    values = (3, 1, 3)   # a repeated value is drawn again, from the stream of its place, into the same file
    r = run(tools["GenerateROIsManyRegions"], "-m", mp, "-o", base, "-n", 17, "-x", 5, "-y", 4, "-z", 3,
            *sum((["-M", v] for v in values), []))
    assert r.returncode == 0, r.stderr
    want, _ = S.random_rois(mask, 17, (5, 4, 3), values=values, per_value=True, seed=SEED)
    assert sorted(os.listdir(str(tmp_path))) == ["many_1.ROIInfo", "many_3.ROIInfo", "mask.nii.gz"]
    assert (tmp_path / "many_1.ROIInfo").read_text().splitlines() == S.roi_info_lines(want[1])
    assert (tmp_path / "many_3.ROIInfo").read_text().splitlines() == S.roi_info_lines(want[2])
    # without any -M nothing is written and the tool succeeds
    r = run(tools["GenerateROIsManyRegions"], "-m", mp, "-o", str(tmp_path / "none_"))
    assert r.returncode == 0 and len(os.listdir(str(tmp_path))) == 3
    # one absent value fails the call: no file
    r = run(tools["GenerateROIsManyRegions"], "-m", mp, "-o", str(tmp_path / "bad_"), "-x", 1, "-y", 1, "-z", 1,
            "-M", 1, "-M", 9)
    assert r.returncode != 0 and "Failed to generate ROIs." in r.stderr and "set 1" in r.stderr
    assert len(os.listdir(str(tmp_path))) == 3


@pytest.mark.gpu
def test_sample_rois_csv_equals_numpy(tools, tmp_path):
    rng = np.random.default_rng(72)
    img = rng.normal(-500, 300, SHAPE).astype(np.float32)
    img[0, 0, :4] = [0.0, -0.0, 1e-7, 123456789.0]
    ip = str(tmp_path / "img.nii")
    niftiio.write(ip, img)
    boxes = [[0, 0, 0, 67, 2, 2], [3, 9, 7, 67, 2, 2], [1, 4, 3, 67, 2, 2], [0, 0, 0, 67, 2, 2]]
    (tmp_path / "rois.txt").write_text("index size\n" + "".join(ln + "\n" for ln in S.roi_info_lines(boxes)))
    out = tmp_path / "bag.csv"
    r = run(tools["SampleROIs"], "-i", ip, "-r", tmp_path / "rois.txt", "-o", out)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["Got 4 rois.", "ROI size [67, 2, 2]."]
    want = S.extract_rois(img, boxes).reshape(4, -1)
    assert out.read_text().splitlines() == [",".join("%g" % v for v in row) for row in want]
    # the same list without a header line, and a box that leaves the image
    (tmp_path / "plain.txt").write_text("".join(ln + "\n" for ln in S.roi_info_lines(boxes)))
    r = run(tools["SampleROIs"], "-i", ip, "-r", tmp_path / "plain.txt", "-o", tmp_path / "p.csv", "-R", "false")
    assert r.returncode == 0 and (tmp_path / "p.csv").read_text() == out.read_text()
    (tmp_path / "outside.txt").write_text("h\n[4, 0, 0][67, 2, 2]\n")
    r = run(tools["SampleROIs"], "-i", ip, "-r", tmp_path / "outside.txt", "-o", tmp_path / "q.csv")
    assert r.returncode != 0 and "Failed to update roiFilter." in r.stderr and not (tmp_path / "q.csv").exists()


@pytest.mark.gpu
def test_make_bag_takes_its_regions_from_the_device_on_request(tools, tmp_path, synth):
    shape = (24, 28, 32)
    img = synth.volume_f32(shape, 401)
    lab = synth.mask_ellipsoids(shape).astype(np.uint16)
    niftiio.write(str(tmp_path / "img.nii.gz"), img)
    niftiio.write(str(tmp_path / "lab.nii.gz"), lab)
    (tmp_path / "hist.txt").write_text("# Features\n# Scales: 1\n" + "-100,0,100\n" * 8)
    os.mkdir(str(tmp_path / "out"))
    args = ["-i", tmp_path / "img.nii.gz", "-m", tmp_path / "lab.nii.gz", "-H", tmp_path / "hist.txt", "-o",
            tmp_path / "out", "-s", 1, "-n", 9, "-x", 7, "-y", 5, "-z", 3]
    r = run(tools["MakeBag"], *args, "-p", "dev", IFE_DEVICE_SAMPLING="1")
    assert r.returncode == 0, r.stderr
    want, _ = S.random_rois(lab, 9, (7, 5, 3), seed=SEED)
    assert (tmp_path / "out" / "dev.ROIInfo").read_text().splitlines() == S.roi_info_lines(want[0])
    assert len((tmp_path / "out" / "dev.bag").read_text().splitlines()) == 9
    # unset (or "0") the host generator draws as before: other boxes, the same number
    r = run(tools["MakeBag"], *args, "-p", "host", IFE_DEVICE_SAMPLING="0")
    assert r.returncode == 0, r.stderr
    host = (tmp_path / "out" / "host.ROIInfo").read_text().splitlines()
    assert len(host) == 9 and host != S.roi_info_lines(want[0])


@pytest.mark.gpu
def test_edges_tool_draws_on_the_device_on_request(tools, tmp_path, synth):
    """-S under IFE_DEVICE_SAMPLING=1: repeatable under IFE_SEED, other positions than the host
    generator's, edges non-decreasing and inside the range of -S 0; a mask without foreground
    fails with the tool's message."""
    tool = os.path.join(BIN, "DetermineHistogramBinEdges_MultiScaleEigenvalueFeatures")
    shape = (16, 20, 24)
    niftiio.write(str(tmp_path / "img.nii.gz"), synth.volume_f32(shape, 300))
    niftiio.write(str(tmp_path / "lab.nii.gz"), synth.mask_ellipsoids(shape))
    niftiio.write(str(tmp_path / "none.nii.gz"), np.zeros(shape, np.uint8))
    (tmp_path / "pairs.csv").write_text("%s , %s\n\n" % (tmp_path / "img.nii.gz", tmp_path / "lab.nii.gz"))
    (tmp_path / "empty.csv").write_text("%s , %s\n\n" % (tmp_path / "img.nii.gz", tmp_path / "none.nii.gz"))

    def edges(name, samples, pairs="pairs.csv", **env):
        r = run(tool, "-i", tmp_path / pairs, "-o", tmp_path / name, "-b", 7, "-s", 1, "-s", 2.5, "-f", 1, "-f", 2,
                "-S", samples, **env)
        return r, ((tmp_path / name).read_text() if r.returncode == 0 else None)

    r, dev = edges("dev.txt", 300, IFE_DEVICE_SAMPLING="1")
    assert r.returncode == 0, r.stderr
    assert edges("dev2.txt", 300, IFE_DEVICE_SAMPLING="1")[1] == dev
    assert edges("host.txt", 300)[1] != dev
    whole = [[float(x) for x in ln.split(",")] for ln in edges("all.txt", 0)[1].splitlines()[2:]]
    rows = [[float(x) for x in ln.split(",")] for ln in dev.splitlines()[2:]]
    assert len(rows) == 16 and all(len(row) == 6 and row == sorted(row) for row in rows)
    # the two scales of an image draw from streams of their own: their smoothed values differ anyway,
    # so compare the spread with the exhaustive edges instead
    for row, ref in zip(rows, whole):
        span = ref[-1] - ref[0]
        assert ref[0] - span <= row[0] and row[-1] <= ref[-1] + span
    r, _ = edges("none.txt", 300, pairs="empty.csv", IFE_DEVICE_SAMPLING="1")
    assert r.returncode != 0 and "No foreground voxel in mask" in r.stderr
