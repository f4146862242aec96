"""CPU test of the sampling binding: the three entry points are exported and listed, their ctypes
signatures have the argument counts include/ife_hip.h declares, the Context methods exist, and
the refusals that need no device (no compute call)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ife_hip.h")
ENTRY_POINTS = {"ife_sample_positions": 15, "ife_random_rois": 15, "ife_extract_rois": 8}


def declared_argument_count(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, re.S)
    assert m, "%s is not declared in ife_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_symbol_is_exported_with_the_header_signature(ife, name):
    lib = ife.load_library()
    assert name in ife.EXPORTS and ife.EXPORTS.count(name) == 1
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared_argument_count(name) == ENTRY_POINTS[name]


def test_draw_argtypes_are_unsigned_where_the_header_is(ife):
    lib = ife.load_library()
    for fn in (lib.ife_sample_positions, lib.ife_random_rois):
        assert fn.argtypes[8] is C.c_uint64 and fn.argtypes[9] is C.c_uint32 and fn.argtypes[10] is C.c_uint64
        assert fn.argtypes[11] is C.c_int64


def test_exports_are_complete(ife):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ife_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(ife.EXPORTS) == declared
    assert int(re.search(r"#define IFE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 1


def test_context_methods_exist(ife):
    draw = ["n_draws", "size", "values", "per_value", "seed", "stream", "first_draw"]
    for method, args in (("sample_positions", ["mask"] + draw),
                         ("random_rois", ["mask"] + draw),
                         ("sample_positions_device", ["mask_ptr", "dtype", "shape_zyx", "out_ptr"] + draw),
                         ("random_rois_device", ["mask_ptr", "dtype", "shape_zyx", "out_ptr"] + draw),
                         ("extract_rois", ["src", "rois"]),
                         ("extract_rois_device", ["src_ptr", "elem_bytes", "src_shape_zyx", "rois_ptr", "n_rois",
                                                  "dst_ptr"])):
        fn = getattr(ife.Context, method, None)
        assert callable(fn), method
        params = inspect.signature(fn).parameters
        assert all(a in params for a in args), (method, list(params))
    p = inspect.signature(ife.Context.sample_positions).parameters
    assert tuple(p["size"].default) == (1, 1, 1) and p["per_value"].default is False
    assert p["seed"].default == p["stream"].default == p["first_draw"].default == 0


def test_a_null_context_is_refused(ife):
    lib = ife.load_library()
    vol = np.ones((2, 2, 2), np.uint8)
    d = ife._desc(vol.shape, (1.0, 1.0, 1.0))
    out = np.full(6, 9, np.int64)
    counts = (C.c_int64 * 1)(-1)
    for fn in (lib.ife_sample_positions, lib.ife_random_rois):
        assert fn(None, vol.ctypes.data, ife.U8, C.byref(d), None, 0, 0, None, 1, 0, 0, 1, out.ctypes.data, counts,
                  ife.MEM_HOST) == ife.E_ARG
    assert (out == 9).all() and counts[0] == -1
    rois = np.array([0, 0, 0, 1, 1, 1], np.int64)
    dst = np.full(1, 9, np.uint8)
    assert lib.ife_extract_rois(None, vol.ctypes.data, 1, C.byref(d), rois.ctypes.data, 1, dst.ctypes.data,
                                ife.MEM_HOST) == ife.E_ARG
    assert dst[0] == 9


class _NoDevice:
    """Stands in for a Context: the argument refusals of the methods come before any call."""
    _lib = None
    _h = None

    def _chk(self, rc):
        raise AssertionError("the library was called")


def test_python_refusals_need_no_device(ife):
    nd = _NoDevice()
    m8, m16 = np.ones((3, 4, 5), np.uint8), np.ones((3, 4, 5), np.uint16)
    for fn in (ife.Context.sample_positions, ife.Context.random_rois):
        with pytest.raises(ValueError):   # a value outside the dtype's range
            fn(nd, m8, 1, (1, 1, 1), values=[256])
        with pytest.raises(ValueError):
            fn(nd, m16, 1, (1, 1, 1), values=[65536])
        with pytest.raises(ValueError):
            fn(nd, m8, 1, (1, 1, 1), values=[-1])
        with pytest.raises(ValueError):   # per_value without a value
            fn(nd, m8, 1, (1, 1, 1), per_value=True)
        with pytest.raises(ValueError):   # 33 values
            fn(nd, m8, 1, (1, 1, 1), values=[1] * 33)
        with pytest.raises(ValueError):   # a size of 0
            fn(nd, m8, 1, (1, 0, 1))
        with pytest.raises(ValueError):   # a negative count
            fn(nd, m8, -1, (1, 1, 1))
        with pytest.raises(ValueError):   # the seed has 64 bits, the stream 32
            fn(nd, m8, 1, (1, 1, 1), seed=2 ** 64)
        with pytest.raises(ValueError):
            fn(nd, m8, 1, (1, 1, 1), stream=2 ** 32)
        with pytest.raises(ValueError):
            fn(nd, m8, 1, (1, 1, 1), first_draw=-1)
        with pytest.raises(TypeError):
            fn(nd, m8.astype(np.int16), 1, (1, 1, 1))
        with pytest.raises(ValueError):
            fn(nd, m8[0], 1, (1, 1, 1))
    with pytest.raises(TypeError):
        ife.Context.sample_positions_device(nd, 256, ife.F32, (3, 4, 5), 512, 1)
    with pytest.raises(TypeError):
        ife.Context.random_rois_device(nd, 256, ife.I16, (3, 4, 5), 512, 1)
    with pytest.raises(TypeError):    # elem_bytes 3
        ife.Context.extract_rois(nd, np.zeros((2, 2, 2), "V3"), [[0, 0, 0, 1, 1, 1]])
    with pytest.raises(TypeError):
        ife.Context.extract_rois_device(nd, 256, 3, (2, 2, 2), 512, 1, 1024)
    with pytest.raises(ValueError):
        ife.Context.extract_rois_device(nd, 256, 4, (2, 2, 2), 512, -1, 1024)
    with pytest.raises(ValueError):
        ife.Context.extract_rois(nd, np.zeros((3, 4), np.float32), [[0, 0, 0, 1, 1, 1]])
    with pytest.raises(ValueError):
        ife.Context.extract_rois(nd, np.zeros((3, 4, 5), np.float32), [[0, 0, 0, 1, 0, 1]])
    assert ife.Context.extract_rois(nd, np.zeros((3, 4, 5), np.float32), np.empty((0, 6))).shape[0] == 0
