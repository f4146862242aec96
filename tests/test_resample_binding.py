"""CPU test of the resampling binding: both entry points are exported and declared, their ctypes
signatures have the argument counts include/ife_hip.h declares, the interpolation constants agree
with the header, and the Context methods exist with the named parameters (no compute call)."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ife_hip.h")
ENTRY_POINTS = ("ife_resample", "ife_resample_f64")


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


def test_interpolation_constants_agree(ife):
    m = re.search(r"IFE_INTERP_LINEAR\s*=\s*(\d+)\s*,\s*IFE_INTERP_NEAREST\s*=\s*(\d+)", _header())
    assert m and (ife.INTERP_LINEAR, ife.INTERP_NEAREST) == (int(m.group(1)), int(m.group(2))) == (0, 1)
    assert "#define IFE_ABI_VERSION 1\n" in open(HEADER).read()


def test_context_methods_exist(ife):
    geometry = ["src_spacing", "src_origin", "dst_shape", "dst_spacing", "dst_origin", "translation",
                "interpolation", "default"]
    for method, args in (("resample", ["src"] + geometry),
                         ("resample_device", ["src_ptr", "src_dtype", "src_shape", "out_ptr"] + geometry)):
        fn = getattr(ife.Context, method, None)
        assert callable(fn), method
        params = inspect.signature(fn).parameters
        assert all(a in params for a in args), (method, list(params))
    p = inspect.signature(ife.Context.resample).parameters
    assert tuple(p["translation"].default) == (0, 0, 0) and p["interpolation"].default == ife.INTERP_LINEAR
    assert p["default"].default == 0.0
