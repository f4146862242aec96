"""IFE_OPT_DIFFERENTIAL across the layers that need no device: the C header, the Python binding
and the host tools, which reach the option through ife::host::Engine (IFE_DIFFERENTIAL)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "image-feature-extraction_amd")
HOST = os.path.join(PKG_DIR, "host")
TOOLS = ["ExtractFeatures", "DetermineHistogramBinEdges_MultiScaleEigenvalueFeatures", "MakeBag", "MakeBagDense",
         "MakeBagOnlyIntensity"]


def header_options():
    text = open(os.path.join(ROOT, "include", "ife_hip.h")).read()
    body = text[text.index("/* Options for ife_ctx_set_option */"):text.index("} ife_option;")]
    return {name: int(value) for name, value in re.findall(r"\b(IFE_OPT_[A-Z_]+) = (\d+)", body)}


def test_header_defines_the_option():
    opts = header_options()
    assert opts["IFE_OPT_DIFFERENTIAL"] == 13
    assert sorted(opts.values()) == list(range(1, 14)), "option values are dense and unique"


def test_binding_constants_equal_the_header(ife):
    opts = header_options()
    assert ife.OPT_DIFFERENTIAL == opts["IFE_OPT_DIFFERENTIAL"] == 13
    for name, value in opts.items():
        assert getattr(ife, name[len("IFE_"):]) == value, name


def test_host_tools_still_build():
    """The engine and the feature filter changed under every tool: all of them compile and link, and
    answer --help without touching a device."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG_DIR, "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    for tool in TOOLS:
        r = subprocess.run([os.path.join(HOST, "bin", tool), "--help"], capture_output=True, text=True,
                           env=dict(os.environ, IFE_DIFFERENTIAL="1"))
        assert r.returncode == 0, (tool, r.stderr)
