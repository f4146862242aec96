"""CPU test of the dense bag binding: the three Context methods exist and the ctypes signatures
of their entry points have the argument counts include/ife_hip.h declares (no compute call)."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ife_hip.h")
ENTRY_POINTS = ("ife_dense_rois", "ife_dense_roi_histograms", "ife_bag_image_dense")


def declared_argument_count(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, re.S)
    assert m, "%s is not declared in ife_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_ctypes_signature_matches_header(ife, name):
    lib = ife.load_library()
    assert name in ife.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared_argument_count(name)


def test_context_methods_exist(ife):
    for method, args in (("dense_rois", ["mask", "size"]),
                         ("dense_roi_histograms", ["features", "mask", "size", "edges", "gen_mask", "layout"]),
                         ("bag_image_dense", ["image", "mask", "sigmas", "size", "edges", "gen_mask", "spacing"])):
        fn = getattr(ife.Context, method, None)
        assert callable(fn), method
        params = inspect.signature(fn).parameters
        assert all(a in params for a in args), (method, list(params))
    assert ife.OPT_DENSE_SCRATCH_MB == int(re.search(r"IFE_OPT_DENSE_SCRATCH_MB\s*=\s*(\d+)",
                                                     open(HEADER).read()).group(1))
