"""CPU-side checks of the weighted queries of a source group (dppr_group_topk_weighted, dppr_group_score_at): declared in
include/dppr.h with the exact definition of the score, exported by the library, prototypes set, and the Python wrappers refuse
malformed weights before they call into the library. No GPU call is made."""
import ctypes
import os
import re

import numpy as np
import pytest

from dynamicppr_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = ("dppr_group_topk_weighted", "dppr_group_score_at")


def test_header_declares_the_queries_and_defines_the_score():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in QUERIES:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)  # backward compatible additions
    flat = " ".join(text.split())
    assert "acc = w[j][0] * p_0[v]" in flat and "acc = acc + w[j][i] * p_i[v]" in flat
    assert "nothing is fused" in flat


def test_library_exports_the_queries_and_prototypes_are_set():
    lib = ctypes.CDLL(eng.build())
    for name in QUERIES:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    L = eng.lib()
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    ip, dp = ctypes.POINTER(i32), ctypes.POINTER(dbl)
    assert list(L.dppr_group_topk_weighted.argtypes) == [vp, i32, dp, i32, i32, dbl, ip, dp, ip]
    assert list(L.dppr_group_score_at.argtypes) == [vp, i32, dp, i32, ip, i32, dp]
    assert L.dppr_group_topk_weighted.restype is ctypes.c_int and L.dppr_group_score_at.restype is ctypes.c_int


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    w = (ctypes.c_double * 2)(1.0, 1.0)
    ids = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    sc = (ctypes.c_double * 4)(1.5, 1.5, 1.5, 1.5)
    cnt = ctypes.c_int32(-7)
    assert L.dppr_group_topk_weighted(None, 0, w, 1, 4, 0.0, ids, sc, ctypes.byref(cnt)) == -1
    assert L.dppr_group_score_at(None, 0, w, 1, ids, 4, sc) == -1
    assert list(ids) == [7] * 4 and list(sc) == [1.5] * 4 and cnt.value == -7


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called into the library ({name}) with malformed weights")


def engine_without_a_device(n):
    e = eng.Engine.__new__(eng.Engine)  # (no dppr_create: only what the wrappers look at before the call)
    e._L, e._h, e._group_n, e.V = _NoLibrary(), None, {0: n}, 64
    return e


@pytest.mark.parametrize("weights", [
    [1.0, 2.0],                              # wrong length for a group of 3
    [[1.0, 2.0, 3.0, 4.0]],                  # wrong trailing dimension
    np.ones((2, 2)),
    np.ones((17, 3)),                        # more than 16 weight vectors
    np.ones((2, 2, 3)),                      # not [n] or [q][n]
    np.zeros((0, 3)),
    [1.0, float("nan"), 0.0],
    [[1.0, 0.0, 0.0], [0.0, float("inf"), 0.0]],
    [0.0, -float("inf"), 0.0],
])
def test_wrappers_refuse_malformed_weights_before_the_library(weights):
    e = engine_without_a_device(3)
    try:
        with pytest.raises(eng.DpprError):
            e.group_topk_weighted(0, weights, 10)
        with pytest.raises(eng.DpprError):
            e.group_score_at(0, weights, [1, 2, 3])
    finally:
        e._h = None  # (nothing to destroy)
