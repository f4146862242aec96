"""CPU test of the scale selection binding: ife_scale_select is exported and listed, its ctypes
signature has the arguments include/ife_hip.h declares, the struct and the constants mirror the
header, the Context methods exist, and the refusals that need no device (no compute call)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ife_hip.h")
NAME = "ife_scale_select"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_symbol_is_exported_with_the_header_signature(ife):
    lib = ife.load_library()
    assert NAME in ife.EXPORTS and ife.EXPORTS.count(NAME) == 1
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, _header(), re.S)
    assert m, "%s is not declared in ife_hip.h" % NAME
    declared = [a.strip() for a in m.group(1).split(",") if a.strip()]
    fn = getattr(lib, NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == len(declared) == 13
    a = fn.argtypes
    assert a[2] is C.c_int and a[4] is C.c_int and a[7] is C.c_int and a[9] is C.c_int and a[12] is C.c_int
    assert a[6] is C.POINTER(C.c_float) and a[8] is C.POINTER(ife.ScaleMeasure)
    assert "float *response" in declared[10] and "uint8_t *scale_index" in declared[11]
    assert "const ife_scale_measure *measures" in declared[8]


def test_exports_are_complete(ife):
    declared = sorted(set(re.findall(r"\b(ife_[a-z0-9_]+)\s*\(", _header())))
    assert sorted(ife.EXPORTS) == declared
    assert int(re.search(r"#define IFE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 1


def test_struct_and_constants_mirror_the_header(ife):
    txt = _header()
    val = lambda name: int(re.search(r"\b%s\s*=\s*(-?\d+)" % name, txt).group(1))  # noqa: E731
    assert (ife.SS_LAPLACIAN, ife.SS_TUBE, ife.SS_PLATE, ife.SS_BLOB) == tuple(
        val(n) for n in ("IFE_SS_LAPLACIAN", "IFE_SS_TUBE", "IFE_SS_PLATE", "IFE_SS_BLOB"))
    assert ife.SS_MAX_MEASURES == int(re.search(r"#define IFE_SS_MAX_MEASURES\s+(\d+)", txt).group(1)) == 4
    body = re.search(r"typedef struct ife_scale_measure \{(.*?)\} ife_scale_measure;", txt, re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(int32_t|float)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [("int32_t", "kind"), ("int32_t", "polarity"), ("float", "gamma"), ("float", "alpha"),
                      ("float", "beta"), ("float", "c")]
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, t) for n, t in ife.ScaleMeasure._fields_] == [(n, ctype[t]) for t, n in fields]
    assert C.sizeof(ife.ScaleMeasure) == 24
    m = ife.ScaleMeasure("plate", -1, 0.75, 0.5, 0.25, 15.0)
    assert (m.kind, m.polarity, m.gamma, m.alpha, m.beta, m.c) == (ife.SS_PLATE, -1, 0.75, 0.5, 0.25, 15.0)
    assert ife.SS_KIND_NAMES == ("laplacian", "tube", "plate", "blob")
    with pytest.raises(ValueError):
        ife.ScaleMeasure("vessel")


def test_context_methods_exist(ife):
    for method, args in (("scale_select", ["image", "mask", "sigmas", "measures", "spacing", "want_index"]),
                         ("scale_select_device", ["image_ptr", "image_dtype", "mask_ptr", "mask_dtype", "shape_zyx",
                                                  "spacing", "sigmas", "measures", "response_ptr", "index_ptr"])):
        fn = getattr(ife.Context, method, None)
        assert callable(fn), method
        params = inspect.signature(fn).parameters
        assert all(a in params for a in args), (method, list(params))
    assert inspect.signature(ife.Context.scale_select).parameters["want_index"].default is True


def test_a_null_context_is_refused(ife):
    lib = ife.load_library()
    img = np.ones((4, 4, 4), np.float32)
    d = ife._desc(img.shape, (1.0, 1.0, 1.0))
    ms = (ife.ScaleMeasure * 1)(ife.ScaleMeasure(ife.SS_LAPLACIAN))
    resp, idx = np.full(64, 9, np.float32), np.full(64, 9, np.uint8)
    rc = lib.ife_scale_select(None, img.ctypes.data, ife.F32, None, ife.U8, C.byref(d), ife._sigma_arg([1.0]), 1, ms, 1,
                              resp.ctypes.data, idx.ctypes.data, ife.MEM_HOST)
    assert rc == ife.E_ARG and (resp == 9).all() and (idx == 9).all()


class _NoDevice:
    """Stands in for a Context: the argument refusals of the methods come before any call."""
    _lib = None
    _h = None

    def _chk(self, rc):
        raise AssertionError("the library was called")


def test_python_refusals_need_no_device(ife):
    nd = _NoDevice()
    img, msk = np.zeros((4, 5, 6), np.float32), np.ones((4, 5, 6), np.uint8)
    good = ife.ScaleMeasure(ife.SS_TUBE, 1, 1.0, 0.5, 0.5, 15.0)
    bad = [[], [good] * 5,
           [ife.ScaleMeasure(7)], [ife.ScaleMeasure(ife.SS_TUBE, 0)], [ife.ScaleMeasure(ife.SS_TUBE, 2)],
           [ife.ScaleMeasure(ife.SS_LAPLACIAN, 1, -1.0)], [ife.ScaleMeasure(ife.SS_LAPLACIAN, 1, float("nan"))],
           [ife.ScaleMeasure(ife.SS_LAPLACIAN, 1, float("inf"))],
           [good, ife.ScaleMeasure(ife.SS_PLATE, 1, 1.0, 0.0, 0.5, 1.0)],
           [good, ife.ScaleMeasure(ife.SS_BLOB, 1, 1.0, 0.5, -0.5, 1.0)],
           [good, ife.ScaleMeasure(ife.SS_TUBE, 1, 1.0, 0.5, 0.5, float("inf"))],
           [good, ife.ScaleMeasure(ife.SS_TUBE, 1, 1.0, 0.5, 0.5, 1e-60)]]       # zero as a float
    for ms in bad:
        with pytest.raises(ValueError):
            ife.Context.scale_select(nd, img, msk, [1.0, 2.0], ms)
        with pytest.raises(ValueError):
            ife.Context.scale_select_device(nd, 256, ife.F32, 512, ife.U8, img.shape, (1.0, 1.0, 1.0), [1.0], ms, 1024)
    with pytest.raises(ValueError):   # 256 scales: index 255 is taken
        ife.Context.scale_select(nd, img, msk, [1.0] * 256, [good])
    with pytest.raises(ValueError):
        ife.Context.scale_select(nd, img[0], msk[0], [1.0], [good])
    with pytest.raises(TypeError):
        ife.Context.scale_select(nd, img, msk.astype(np.int32), [1.0], [good])
    # measures may be given as dicts and tuples too; LAPLACIAN ignores alpha, beta and c
    arr = ife._scale_measures_arg([dict(kind="blob", polarity=-1, c=3.0), ("laplacian", 1, 0.75, -1.0, 0.0, -3.0), good], 255)
    assert [m.kind for m in arr] == [ife.SS_BLOB, ife.SS_LAPLACIAN, ife.SS_TUBE] and arr[0].c == 3.0
