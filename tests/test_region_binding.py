"""CPU test of the region binding: the Context methods exist, the ctypes signatures of the three
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
ENTRY_POINTS = {"ife_mask_bounding_box": 7, "ife_extract_region": 10, "ife_label_membership": 10}


def declared_argument_count(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, re.S)
    assert m, "%s is not declared in ife_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_ctypes_signature_matches_header(ife, name):
    lib = ife.load_library()
    assert name in ife.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared_argument_count(name) == ENTRY_POINTS[name]


def test_context_methods_exist(ife):
    for method, args in (("mask_bounding_box", ["mask"]),
                         ("mask_bounding_box_device", ["ptr", "dtype", "shape_zyx"]),
                         ("extract_region", ["src", "index_xyz", "size_xyz", "pad_value", "flip"]),
                         ("extract_region_device", ["src_ptr", "elem_bytes", "src_shape_zyx", "index_xyz", "size_xyz",
                                                    "dst_ptr", "pad_value", "flip"]),
                         ("label_membership", ["labels", "include", "inside", "outside"]),
                         ("label_membership_device", ["labels_ptr", "dtype", "n", "include", "out_ptr", "inside",
                                                      "outside"])):
        fn = getattr(ife.Context, method, None)
        assert callable(fn), method
        params = inspect.signature(fn).parameters
        assert all(a in params for a in args), (method, list(params))
    p = inspect.signature(ife.Context.extract_region).parameters
    assert p["pad_value"].default is None and tuple(p["flip"].default) == (False, False, False)
    p = inspect.signature(ife.Context.label_membership).parameters
    assert p["inside"].default == 1 and p["outside"].default == 0


def test_abi_and_kernel_kinds_are_not_raised(ife):
    """New symbols are additions: the ABI version stays 1 and the launches are accounted under
    the existing kinds."""
    txt = open(HEADER).read()
    assert int(re.search(r"#define IFE_ABI_VERSION\s+(\d+)", txt).group(1)) == 1
    assert ife.MAX_KERNEL_KINDS == 24 == int(re.search(r"#define IFE_MAX_KERNEL_KINDS\s+(\d+)", txt).group(1))


def test_a_null_context_is_refused(ife):
    lib = ife.load_library()
    vol = np.ones((2, 2, 2), np.uint8)
    d = ife._desc(vol.shape, (1.0, 1.0, 1.0))
    box = (C.c_int64 * 6)(*([9] * 6))
    count = C.c_int64(-1)
    assert lib.ife_mask_bounding_box(None, vol.ctypes.data, ife.U8, C.byref(d), box, C.byref(count),
                                     ife.MEM_HOST) == ife.E_ARG
    assert list(box) == [9] * 6 and count.value == -1
    out = np.full(8, 9, np.uint8)
    region = (C.c_int64 * 6)(0, 0, 0, 2, 2, 2)
    assert lib.ife_extract_region(None, vol.ctypes.data, 1, C.byref(d), region, 0, None, out.ctypes.data,
                                  ife.MEM_HOST, ife.MEM_HOST) == ife.E_ARG
    inc = (C.c_int * 1)(1)
    assert lib.ife_label_membership(None, vol.ctypes.data, ife.U8, 8, inc, 1, 1, 0, out.ctypes.data,
                                    ife.MEM_HOST) == ife.E_ARG
    assert (out == 9).all()


class _NoDevice:
    """Stands in for a Context: the argument refusals of the methods come before any call."""
    _lib = None
    _h = None

    def _chk(self, rc):
        raise AssertionError("the library was called")


def test_python_refusals_need_no_device(ife):
    nd = _NoDevice()
    src = np.zeros((3, 4, 5), np.float32)
    with pytest.raises(TypeError):    # elem_bytes 3
        ife.Context.extract_region(nd, np.zeros((2, 2, 2), "V3"), (0, 0, 0), (1, 1, 1))
    with pytest.raises(TypeError):
        ife.Context.extract_region_device(nd, 256, 3, (2, 2, 2), (0, 0, 0), (1, 1, 1), 512)
    with pytest.raises(ValueError):   # a size of 0
        ife.Context.extract_region(nd, src, (0, 0, 0), (5, 0, 3))
    with pytest.raises(ValueError):   # flip 8
        ife.Context.extract_region(nd, src, (0, 0, 0), (1, 1, 1), flip=8)
    with pytest.raises(ValueError):   # a NULL pad value with a region that reaches outside
        ife.Context.extract_region(nd, src, (-1, 0, 0), (2, 1, 1))
    with pytest.raises(ValueError):
        ife.Context.extract_region(nd, src, (4, 0, 0), (2, 1, 1), flip=(True, False, False))
    with pytest.raises(ValueError):
        ife.Context.extract_region(nd, np.zeros((3, 4), np.float32), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):   # an include value of 256 for uint8
        ife.Context.label_membership(nd, np.zeros(4, np.uint8), [1, 256])
    with pytest.raises(ValueError):
        ife.Context.label_membership(nd, np.zeros(4, np.uint8), [1], inside=256)
    with pytest.raises(ValueError):
        ife.Context.label_membership(nd, np.zeros(4, np.uint16), [1], outside=-1)
    with pytest.raises(ValueError):
        ife.Context.label_membership_device(nd, 256, ife.U16, 4, [65536], 512)
    with pytest.raises(TypeError):
        ife.Context.label_membership(nd, np.zeros(4, np.int16), [1])
    with pytest.raises(TypeError):
        ife.Context.mask_bounding_box(nd, np.zeros((2, 2, 2), np.float64))
    with pytest.raises(ValueError):
        ife.Context.mask_bounding_box(nd, np.zeros((2, 2), np.uint8))
