"""CPU test of the dense bag stream's binding: the three entry points are exported, their ctypes
signatures have the argument counts include/ife_hip.h declares, and the generator method and the
two value constants exist (no compute call)."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ife_hip.h")
ENTRY_POINTS = ("ife_bag_dense_stream_begin", "ife_bag_dense_stream_next", "ife_bag_dense_stream_end")


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


def test_argument_counts_are_the_documented_ones():
    assert [declared_argument_count(n) for n in ENTRY_POINTS] == [18, 5, 1]


def test_generator_and_constants_exist(ife):
    fn = getattr(ife.Context, "bag_image_dense_stream", None)
    assert callable(fn) and inspect.isgeneratorfunction(fn)
    params = inspect.signature(fn).parameters
    for a in ("image", "mask", "sigmas", "size", "edges", "gen_mask", "spacing", "values", "block_mb"):
        assert a in params, (a, list(params))
    assert params["values"].default == "frequencies" and params["block_mb"].default == 0
    txt = open(HEADER).read()
    for name, value in (("IFE_BAG_COUNTS", ife.BAG_COUNTS), ("IFE_BAG_FREQUENCIES", ife.BAG_FREQUENCIES)):
        assert value == int(re.search(r"\b%s\s*=\s*(\d+)" % name, txt).group(1))
