"""CPU test of the census and coverage binding: the three entry points are exported and listed,
their ctypes signatures have the argument counts include/ife_hip.h declares, the Context methods
exist, and the refusals that need no device (no compute call)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ife_hip.h")
# ife_value_census_f32(ctx, values, n, uniq, counts, capacity, n_unique, n_nan, mem) has nine
ENTRY_POINTS = {"ife_value_census_f32": 9, "ife_threshold_mask": 8, "ife_roi_coverage": 12}


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


def test_argtypes_are_the_header_types(ife):
    lib = ife.load_library()
    p64 = C.POINTER(C.c_int64)
    a = lib.ife_value_census_f32.argtypes
    assert a[2] is C.c_int64 and a[5] is C.c_int64 and a[6] is p64 and a[7] is p64 and a[8] is C.c_int
    a = lib.ife_threshold_mask.argtypes
    assert a[2] is C.c_int64 and a[3] is C.c_float and a[4] is C.c_float and a[6] is p64
    a = lib.ife_roi_coverage.argtypes
    assert a[2] is C.c_int and a[5] is C.c_int64 and a[6] is p64 and a[7] is C.c_int
    assert a[8] is p64 and a[9] is p64 and a[10] is p64
    # the counts of the census are uint32 in the header and in what the method returns
    txt = open(HEADER).read()
    assert re.search(r"ife_value_census_f32\([^)]*float \*uniq, uint32_t \*counts,\s*int64_t capacity", txt)


def test_exports_are_complete(ife):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ife_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(ife.EXPORTS) == declared
    assert int(re.search(r"#define IFE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 1
    assert int(re.search(r"#define IFE_MAX_KERNEL_KINDS\s+(\d+)", open(HEADER).read()).group(1)) == 24


def test_context_methods_exist(ife):
    for method, args in (("value_census", ["values"]),
                         ("value_census_device", ["values_ptr", "n", "uniq_ptr", "counts_ptr", "capacity"]),
                         ("threshold_mask", ["image", "low", "high"]),
                         ("threshold_mask_device", ["image_ptr", "n", "low", "high", "mask_ptr"]),
                         ("roi_coverage", ["mask", "rois", "round_ends"]),
                         ("roi_coverage_device", ["mask_ptr", "dtype", "shape_zyx", "rois_ptr", "n_rois",
                                                  "round_ends"])):
        fn = getattr(ife.Context, method, None)
        assert callable(fn), method
        params = inspect.signature(fn).parameters
        assert all(a in params for a in args), (method, list(params))


def test_a_null_context_is_refused(ife):
    lib = ife.load_library()
    v = np.ones(4, np.float32)
    u, c = np.full(4, 9, np.float32), np.full(4, 9, np.uint32)
    nu, nn = C.c_int64(-1), C.c_int64(-1)
    assert lib.ife_value_census_f32(None, v.ctypes.data, 4, u.ctypes.data, c.ctypes.data, 4, C.byref(nu), C.byref(nn),
                                    ife.MEM_HOST) == ife.E_ARG
    assert (u == 9).all() and (c == 9).all() and nu.value == nn.value == -1
    m = np.full(4, 9, np.uint8)
    assert lib.ife_threshold_mask(None, v.ctypes.data, 4, 0.0, 1.0, m.ctypes.data, C.byref(nu), ife.MEM_HOST) == ife.E_ARG
    assert (m == 9).all() and nu.value == -1
    d = ife._desc((1, 2, 2), (1.0, 1.0, 1.0))
    rois = np.array([0, 0, 0, 1, 1, 1], np.int64)
    ends = (C.c_int64 * 1)(1)
    vis, hit = (C.c_int64 * 1)(-1), (C.c_int64 * 1)(-1)
    assert lib.ife_roi_coverage(None, m.ctypes.data, ife.U8, C.byref(d), rois.ctypes.data, 1, ends, 1, vis, hit,
                                C.byref(nu), ife.MEM_HOST) == ife.E_ARG
    assert vis[0] == hit[0] == nu.value == -1


class _NoDevice:
    """Stands in for a Context: the argument refusals of the methods come before any call."""
    _lib = None
    _h = None

    def _chk(self, rc):
        raise AssertionError("the library was called")


def test_python_refusals_need_no_device(ife):
    nd = _NoDevice()
    f32, m8 = np.zeros((3, 4, 5), np.float32), np.ones((3, 4, 5), np.uint8)
    box = [[0, 0, 0, 1, 1, 1]]
    with pytest.raises(TypeError):    # wrong dtypes
        ife.Context.value_census(nd, f32.astype(np.float64))
    with pytest.raises(TypeError):
        ife.Context.value_census(nd, f32.astype(np.int16))
    with pytest.raises(ValueError):
        ife.Context.value_census(nd, f32[:0])
    with pytest.raises(ValueError):
        ife.Context.value_census_device(nd, 256, 0)
    with pytest.raises(ValueError):
        ife.Context.value_census_device(nd, 256, 4, 512, 1024, -1)
    with pytest.raises(TypeError):
        ife.Context.threshold_mask(nd, f32.astype(np.float64), 0.0, 1.0)
    with pytest.raises(ValueError):   # low > high
        ife.Context.threshold_mask(nd, f32, 2.0, 1.0)
    with pytest.raises(ValueError):   # two denormals, low > high
        ife.Context.threshold_mask(nd, f32, 3e-45, 1e-45)
    with pytest.raises(ValueError):
        ife.Context.threshold_mask(nd, f32, float("nan"), 1.0)
    with pytest.raises(ValueError):
        ife.Context.threshold_mask_device(nd, 256, 4, 2.0, 1.0, 512)
    with pytest.raises(ValueError):
        ife.Context.threshold_mask_device(nd, 256, 4, 0.0, float("nan"), 512)
    with pytest.raises(ValueError):
        ife.Context.threshold_mask_device(nd, 256, 0, 0.0, 1.0, 512)
    with pytest.raises(TypeError):
        ife.Context.roi_coverage(nd, m8.astype(np.int16), box, [1])
    with pytest.raises(TypeError):
        ife.Context.roi_coverage(nd, f32, box, [1])
    with pytest.raises(ValueError):
        ife.Context.roi_coverage(nd, m8[0], box, [1])
    with pytest.raises(ValueError):   # rois not [n][6]
        ife.Context.roi_coverage(nd, m8, [[0, 0, 0, 1, 1]], [1])
    with pytest.raises(ValueError):
        ife.Context.roi_coverage(nd, m8, [0, 0, 0, 1, 1, 1], [1])
    with pytest.raises(ValueError):   # decreasing round ends
        ife.Context.roi_coverage(nd, m8, box * 3, [2, 1])
    with pytest.raises(ValueError):
        ife.Context.roi_coverage(nd, m8, box, [-1, 1])
    with pytest.raises(ValueError):   # an end beyond the boxes
        ife.Context.roi_coverage(nd, m8, box, [2])
    with pytest.raises(ValueError):   # no round, 65 rounds
        ife.Context.roi_coverage(nd, m8, box, [])
    with pytest.raises(ValueError):
        ife.Context.roi_coverage(nd, m8, box, [0] * 65)
    with pytest.raises(TypeError):
        ife.Context.roi_coverage_device(nd, 256, ife.F32, (3, 4, 5), 512, 1, [1])
    with pytest.raises(ValueError):
        ife.Context.roi_coverage_device(nd, 256, ife.U8, (3, 4, 5), 512, -1, [0])
    with pytest.raises(ValueError):
        ife.Context.roi_coverage_device(nd, 256, ife.U16, (3, 4, 5), 512, 3, [2, 1])
