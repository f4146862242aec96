"""The ScaleSpaceFeatures tool (host/tools/ScaleSpaceFeatures.cxx; ours, the reference has no such
tool).  Without a GPU: the flags, the usage and the refusals the tool makes itself.  On the device:
its files, their names, dtypes and geometry; their contents, held equal bit for bit to
Context.scale_select of the same arguments; and the library's refusals as the tools report them."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "image-feature-extraction_amd", "host", "bin", "ScaleSpaceFeatures")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niftiio  # noqa: E402

SHAPE = (9, 11, 37)
SPACING = tuple(float(np.float32(v)) for v in (0.75, 0.75, 1.5))
ORIGIN = (-12.5, 30.25, 4.0)
KIND_NAMES = {"laplacian": "Laplacian", "tube": "Tube", "plate": "Plate", "blob": "Blob"}


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, env=e)


def test_usage_names_every_flag():
    r = _run(["--help"])
    assert r.returncode == 0
    for flag in ("-i", "--image", "-m", "--mask", "-o", "--out", "-s", "--scale", "-k", "--kind", "-p", "--polarity",
                 "-g", "--gamma", "-a", "--alpha", "-b", "--beta", "-c"):
        assert flag in r.stdout, flag
    for word in ("laplacian", "tube", "plate", "blob", "bright", "dark"):
        assert word in r.stdout, word


def test_the_tools_own_refusals(tmp_path):
    base = ["-i", "absent.nii", "-m", "absent.nii", "-o", tmp_path / "o_", "-s", "1"]
    for args, text in ((base[2:] + ["-k", "tube", "-c", "5"], "Error"),                    # -i is required
                       (base[:6] + ["-k", "tube", "-c", "5"], "Error"),                    # -s is required
                       (base, "Error"),                                                    # -k is required
                       (base + ["-k", "vessel"], "Unknown measure: vessel"),
                       (base + ["-k", "tube", "-k", "tube", "-c", "5"], "Measure given twice: tube"),
                       (base + ["-k", "laplacian", "-k", "blob"], "-c is required for tube, plate and blob"),
                       (base + ["-k", "laplacian", "-p", "grey"], "Polarity must be bright or dark"),
                       (base + ["-k", "laplacian", "-g", "one"], "Error"),
                       (base + ["-k", "laplacian"], "Failed to process.")):                # the files are absent
        r = _run(args)
        assert r.returncode == 1 and text in r.stderr, (args, r.stderr)
    assert os.listdir(str(tmp_path)) == []


@pytest.fixture(scope="module")
def files(tmp_path_factory, synth):
    d = tmp_path_factory.mktemp("scale_select_tool")
    image = synth.volume_f32(SHAPE, 7)
    labels = synth.mask_ellipsoids(SHAPE).astype(np.uint8)          # 0, 1 and 2: the tool clamps to {0, 1}
    i, m = str(d / "image.nii"), str(d / "mask.nii.gz")
    niftiio.write(i, image, SPACING, geometry={"qoffset": ORIGIN})
    niftiio.write(m, labels, SPACING, geometry={"qoffset": ORIGIN})
    return d, i, m, image, np.minimum(labels, 1).astype(np.uint8)


def _outputs_equal(ife, prefix, kinds, want, suffix=".nii.gz"):
    for k, kind in enumerate(kinds):
        resp, spacing = niftiio.read(prefix + KIND_NAMES[kind] + "Response" + suffix)
        idx, ispacing = niftiio.read(prefix + KIND_NAMES[kind] + "Scale" + suffix)
        assert resp.dtype == np.float32 and idx.dtype == np.uint8 and resp.shape == idx.shape == SHAPE
        assert spacing == ispacing == SPACING
        for name in ("Response", "Scale"):
            assert niftiio.read_geometry(prefix + KIND_NAMES[kind] + name + suffix)["qoffset"] == ORIGIN
        assert np.array_equal(resp.view(np.uint32), want[0][k].view(np.uint32)), kind
        assert np.array_equal(idx, want[1][k]), kind


@pytest.mark.gpu
def test_files_and_contents_equal_the_context(ife, ctx, files):
    d, i, m, image, mask = files
    sigmas, kinds = [1.0, 1.5, 2.0, 3.0], ["plate", "laplacian", "blob", "tube"]     # the order given is kept
    prefix = str(d / "bright_")
    args = ["-i", i, "-m", m, "-o", prefix, "-g", "0.75", "-a", "0.4", "-b", "0.6", "-c", "60", "-p", "bright"]
    for s in sigmas:
        args += ["-s", s]
    for k in kinds:
        args += ["-k", k]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    made = sorted(f for f in os.listdir(str(d)) if f.startswith("bright_"))
    assert made == sorted("bright_%s%s.nii.gz" % (KIND_NAMES[k], n) for k in kinds for n in ("Response", "Scale"))
    ms = [ife.ScaleMeasure(k, 1, 0.75, 0.4, 0.6, 60.0) for k in kinds]
    want = ctx.scale_select(image, mask, sigmas, ms, spacing=SPACING)
    _outputs_equal(ife, prefix, kinds, want)
    assert (want[1] != 255).sum() > 100
    # one measure, dark, the defaults of -g, -a and -b, another file type
    prefix = str(d / "dark_")
    r = _run(["-i", i, "-m", m, "-o", prefix, "-s", "2", "-s", "1", "-k", "tube", "-c", "60", "-p", "dark"],
             env={"IFE_OUT_FILE_TYPE": ".nii"})
    assert r.returncode == 0, r.stderr
    assert sorted(f for f in os.listdir(str(d)) if f.startswith("dark_")) == ["dark_TubeResponse.nii", "dark_TubeScale.nii"]
    want = ctx.scale_select(image, mask, [2.0, 1.0], [ife.ScaleMeasure("tube", -1, 1.0, 0.5, 0.5, 60.0)], spacing=SPACING)
    _outputs_equal(ife, prefix, ["tube"], want, ".nii")


@pytest.mark.gpu
def test_the_differential_path_through_the_environment(ife, ctx, files):
    d, i, m, image, mask = files
    prefix = str(d / "diff_")
    r = _run(["-i", i, "-m", m, "-o", prefix, "-s", "1", "-s", "2", "-k", "laplacian", "-k", "plate", "-c", "60"],
             env={"IFE_DIFFERENTIAL": "1"})
    assert r.returncode == 0, r.stderr
    ms = [ife.ScaleMeasure("laplacian"), ife.ScaleMeasure("plate", 1, 1.0, 0.5, 0.5, 60.0)]
    plain = ctx.scale_select(image, mask, [1.0, 2.0], ms, spacing=SPACING)
    ctx.set_option(ife.OPT_DIFFERENTIAL, 1)
    try:
        want = ctx.scale_select(image, mask, [1.0, 2.0], ms, spacing=SPACING)
    finally:
        ctx.set_option(ife.OPT_DIFFERENTIAL, 0)
    _outputs_equal(ife, prefix, ["laplacian", "plate"], want)
    assert not np.array_equal(plain[0], want[0])


@pytest.mark.gpu
def test_the_librarys_refusals_as_the_tools_report_them(files):
    d, i, m, _, _ = files
    prefix = str(d / "refused_")
    base = ["-i", i, "-m", m, "-o", prefix]
    for args, word in ((["-s", "1", "-k", "laplacian", "-g", "-1"], "gamma"),
                       (["-s", "1", "-k", "tube", "-c", "0"], "c must"),
                       (["-s", "1", "-k", "plate", "-c", "5", "-a", "0"], "alpha"),
                       (["-s", "1", "-k", "blob", "-c", "5", "-b", "-2"], "beta"),
                       (["-s", "0", "-k", "laplacian"], "sigma"),
                       (["-k", "laplacian"] + ["-s", "1"] * 256, "n_sigmas")):
        r = _run(base + args)
        assert r.returncode == 1 and "Failed to process." in r.stderr and "ExceptionObject" in r.stderr, (args, r.stderr)
        assert word in r.stderr, (args, r.stderr)
    assert not [f for f in os.listdir(str(d)) if f.startswith("refused_")]
