"""CPU test of the label binding: the two Context methods exist, the ctypes signatures of their
entry points have the argument counts include/ife_hip.h declares, and the refusals that need no
device (no compute call)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ife_hip.h")
ENTRY_POINTS = ("ife_roi_labels", "ife_dense_roi_labels")


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
    assert declared_argument_count(name) == {"ife_roi_labels": 11, "ife_dense_roi_labels": 14}[name]


def test_context_methods_exist(ife):
    for method, args in (("roi_labels", ["labels", "rois", "ignore", "dominant"]),
                         ("dense_roi_labels", ["labels", "gen_mask", "size", "ignore", "dominant"])):
        fn = getattr(ife.Context, method, None)
        assert callable(fn), method
        params = inspect.signature(fn).parameters
        assert all(a in params for a in args), (method, list(params))
        assert params["ignore"].default == () and params["dominant"].default == -1


def test_kernel_kinds_are_not_raised(ife):
    """The label launches are accounted under the existing kinds."""
    assert ife.MAX_KERNEL_KINDS == 24 == int(re.search(r"#define IFE_MAX_KERNEL_KINDS\s+(\d+)",
                                                       open(HEADER).read()).group(1))


def test_a_null_context_is_refused(ife):
    lib = ife.load_library()
    lab = np.zeros((2, 2, 2), np.uint8)
    d = ife._desc(lab.shape, (1.0, 1.0, 1.0))
    rois = np.array([[0, 0, 0, 1, 1, 1]], np.int64)
    out = np.full(1, 9, np.uint8)
    n = C.c_int64(-1)
    assert lib.ife_roi_labels(None, lab.ctypes.data, ife.U8, C.byref(d), rois.ctypes.data, 1, None, 0, -1,
                              out.ctypes.data, ife.MEM_HOST) == ife.E_ARG
    assert lib.ife_dense_roi_labels(None, lab.ctypes.data, ife.U8, lab.ctypes.data, ife.U8, C.byref(d),
                                    ife._size_arg((1, 1, 1)), None, 0, -1, out.ctypes.data, 1, C.byref(n),
                                    ife.MEM_HOST) == ife.E_ARG
    assert out[0] == 9 and n.value == -1


class _NoDevice:
    """Stands in for a Context: the argument refusals of the two methods come before any call."""
    _lib = None
    _h = None

    def _chk(self, rc):
        raise AssertionError("the library was called")

    def _dense_count(self, *a, **k):
        raise AssertionError("the library was called")


def test_python_refusals_need_no_device(ife):
    rois = [(0, 0, 0, 1, 1, 1)]
    with pytest.raises(TypeError):
        ife.Context.roi_labels(_NoDevice(), np.zeros((2, 2, 2), np.uint16), rois)
    with pytest.raises(ValueError):
        ife.Context.roi_labels(_NoDevice(), np.zeros((2, 2), np.uint8), rois)
    with pytest.raises(TypeError):
        ife.Context.dense_roi_labels(_NoDevice(), np.zeros((2, 2, 2), np.uint8), None, (1, 1, 1))
    with pytest.raises(TypeError):
        ife.Context.dense_roi_labels(_NoDevice(), np.zeros((2, 2, 2), np.float32), np.ones((2, 2, 2), np.uint8),
                                     (1, 1, 1))
