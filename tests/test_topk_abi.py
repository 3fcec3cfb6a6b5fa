"""CPU-side checks of the state queries (dppr_topk, dppr_group_topk, dppr_read_at, dppr_group_read_at): declared in
include/dppr.h, exported by the library, listed in engine.EXPORTS; no GPU call is made."""
import ctypes
import os
import re

from dynamicppr_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = ("dppr_topk", "dppr_group_topk", "dppr_read_at", "dppr_group_read_at")


def header_text():
    return open(os.path.join(ROOT, "include", "dppr.h")).read()


def test_header_declares_the_queries_and_the_k_limit():
    text = header_text()
    assert re.search(r"^#define DPPR_TOPK_MAX 8192\b", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in QUERIES:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)  # backward compatible additions


def test_library_exports_the_queries():
    lib = ctypes.CDLL(eng.build())
    for name in QUERIES:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ids = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    p = (ctypes.c_double * 4)(1.5, 1.5, 1.5, 1.5)
    cnt = ctypes.c_int32(-7)
    assert L.dppr_topk(None, 0, 4, 0.0, ids, p, None, ctypes.byref(cnt)) == -1
    assert L.dppr_group_topk(None, 0, 4, 0.0, ids, p, None, ctypes.byref(cnt)) == -1
    assert L.dppr_read_at(None, 0, ids, 4, p, None) == -1
    assert L.dppr_group_read_at(None, 0, ids, 4, p, None) == -1
    assert list(ids) == [7] * 4 and list(p) == [1.5] * 4 and cnt.value == -7
