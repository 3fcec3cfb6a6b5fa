"""CPU-side checks of the calls that change a running group's sources (dppr_group_sources, dppr_group_replace_source,
dppr_group_add_source, dppr_group_remove_source): declared in include/dppr.h, exported by the library, listed in engine.EXPORTS,
refused without an engine; no GPU call is made."""
import ctypes
import os
import re

from dynamicppr_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_group_sources", "dppr_group_replace_source", "dppr_group_add_source", "dppr_group_remove_source")


def test_header_declares_the_calls_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)  # backward compatible additions


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert lib.dppr_abi_version() == 6


def test_null_engine_is_rejected_without_a_device():
    L = eng.lib()
    ids = (ctypes.c_int32 * 16)(*([7] * 16))
    n, idx, ms = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_float(-7.0)
    assert L.dppr_group_sources(None, 0, ids, ctypes.byref(n)) == -1
    assert L.dppr_group_replace_source(None, 0, 0, 1, ctypes.byref(ms)) == -1
    assert L.dppr_group_add_source(None, 0, 1, ctypes.byref(idx), ctypes.byref(ms)) == -1
    assert L.dppr_group_remove_source(None, 0, 0) == -1
    assert list(ids) == [7] * 16 and n.value == -7 and idx.value == -7 and ms.value == -7.0
