"""CPU test of the B-spline binding: the five entry points are exported and declared, their ctypes
signatures have the argument counts include/ife_hip.h declares, the constants agree with the header
and the plan, and the Context methods exist with the named parameters (no compute call)."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ife_hip.h")
PLAN = os.path.join(ROOT, "image-feature-extraction_amd", "csrc", "bspline_plan.hpp")
ENTRY_POINTS = ("ife_bspline_coefficients", "ife_bspline_coefficients_f64", "ife_resample_bspline",
                "ife_resample_bspline_f64", "ife_window_u8")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared_argument_count(name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), re.S)
    assert m, "%s is not declared in ife_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_ctypes_signature_matches_header(ife, name):
    lib = ife.load_library()
    assert name in ife.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared_argument_count(name)


def test_constants_agree(ife):
    m = re.search(r"BS_MAX_ORDER\s*=\s*(\d+)", open(PLAN).read())
    assert m and ife.BSPLINE_MAX_ORDER == int(m.group(1)) == 5
    # the enum of ife_resample keeps its two values, and the ABI version stays
    assert re.search(r"typedef enum \{ IFE_INTERP_LINEAR = 0, IFE_INTERP_NEAREST = 1 \} ife_interp;", _header())
    assert "#define IFE_ABI_VERSION 1\n" in open(HEADER).read()


def test_context_methods_exist(ife):
    geometry = ["src_spacing", "src_origin", "dst_shape", "dst_spacing", "dst_origin", "translation", "order",
                "extrapolate", "default"]
    for method, args in (("bspline_coefficients", ["src", "order"]),
                         ("bspline_coefficients_device", ["src_ptr", "src_dtype", "shape_zyx", "order", "coef_ptr"]),
                         ("resample_bspline", ["src"] + geometry),
                         ("resample_bspline_device", ["src_ptr", "src_dtype", "src_shape", "out_ptr"] + geometry),
                         ("window_u8", ["src", "window_min", "window_max", "mask", "out_min", "out_max"]),
                         ("window_u8_device", ["src_ptr", "mask_ptr", "n", "window_min", "window_max", "out_ptr"])):
        fn = getattr(ife.Context, method, None)
        assert callable(fn), method
        params = inspect.signature(fn).parameters
        assert all(a in params for a in args), (method, list(params))
    p = inspect.signature(ife.Context.resample_bspline).parameters
    assert tuple(p["translation"].default) == (0, 0, 0) and p["order"].default == 3
    assert p["extrapolate"].default is False and p["default"].default == 0.0
    assert inspect.signature(ife.Context.bspline_coefficients).parameters["order"].default == 3
