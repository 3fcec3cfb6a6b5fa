"""CPU-side checks of the induced subgraph of a top-k order (dppr_subgraph, dppr_group_subgraph): declared in include/dppr.h with
DPPR_SUBGRAPH_MAX, exported by the library, listed in engine.EXPORTS, rejected without a handle with nothing written; the HIP-free
plan (dynamicppr_amd/csrc/dppr_subgraph_plan.hpp) driven by tests/native/subgraph_plan_test.cpp as a stand-alone program under the
address and undefined-behaviour sanitizers; and the numpy restatement (tests/subgraph_ref.py) against a six-vertex multigraph
counted by hand and against a brute-force double loop on a random multigraph. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_subgraph", "dppr_group_subgraph")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    assert re.search(r"^#define DPPR_SUBGRAPH_MAX DPPR_TOPK_MAX\b", code, re.M)
    assert re.search(r"^#define DPPR_TOPK_MAX 8192\b", code, re.M) and eng.SUBGRAPH_MAX == 8192
    # the contract is stated where a caller reads it
    for phrase in ("as often as it is stored", "IS an edge of the subgraph", "dppr_cluster differs here", "in ascending position",
                   "ABSOLUTE indices", "always written with the TRUE counts", "Prefix property", "Convergence is NOT"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("subgraph", "group_subgraph"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    cnt = np.full(2, 7, dtype=np.int32)
    off = np.full(3, 7, dtype=np.int64)
    ids, col = np.full(8, 7, dtype=np.int32), np.full(8, 7, dtype=np.int32)
    p = np.full(8, 2.5)
    rp = np.full(10, 7, dtype=np.int64)
    for fn in (L.dppr_subgraph, L.dppr_group_subgraph):
        for dest in (eng.DEST_HOST, eng.DEST_DEVICE):
            assert fn(None, 0, -1, 4, 0.0, 8, dest, cnt.ctypes.data, off.ctypes.data, ids.ctypes.data, p.ctypes.data, rp.ctypes.data,
                      col.ctypes.data) == -1
    assert np.all(cnt == 7) and np.all(off == 7) and np.all(ids == 7) and np.all(col == 7) and np.all(p == 2.5) and np.all(rp == 7)


def test_subgraph_plan(tmp_path):
    """dppr_subgraph_plan.hpp: the argument check at its limits, the sizes, the block for every combination of NULLs, subgraph_row."""
    exe = str(tmp_path / "subgraph_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "subgraph_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_subgraph_ref_on_a_graph_counted_by_hand():
    """Six vertices, ten stored edges: 0->1 twice, 1->0, 1->2, the self loop 2->2, 2->3, 3->0, 3->4, 4->5, 5->3. Order 1, 0, 2, 3
    (positions 0, 1, 2, 3):
        row of 1: heads 0, 2     -> 1, 2
        row of 0: heads 1, 1     -> 0, 0      (the duplicate twice)
        row of 2: heads 2, 3     -> 2, 3      (the self loop: its own position)
        row of 3: heads 0, 4     -> 1         (3->4 leaves the order)"""
    V = 6
    row_ptr = np.array([0, 2, 4, 6, 8, 9, 10])
    col = np.array([1, 1, 0, 2, 2, 3, 0, 4, 5, 3])
    order = [1, 0, 2, 3]
    rows = subgraph_ref.rows(V, row_ptr, col, order)
    assert [r.tolist() for r in rows] == [[1, 2], [0, 0], [2, 3], [1]] and all(r.dtype == np.int32 for r in rows)
    assert [r.tolist() for r in subgraph_ref.brute_rows(V, row_ptr, col, order)] == [r.tolist() for r in rows]
    # the stored order inside a row is no part of the rule
    col2 = col.copy()
    col2[2:4] = col[2:4][::-1]
    col2[4:6] = col[4:6][::-1]
    assert [r.tolist() for r in subgraph_ref.rows(V, row_ptr, col2, order)] == [r.tolist() for r in rows]
    # two sources as one CSR, k beyond the second order
    cnt, off, ids, rp, c = subgraph_ref.subgraph(V, row_ptr, col, [order, [5, 3]], 4)
    assert cnt.tolist() == [4, 2] and off.tolist() == [0, 7, 8]
    assert ids.tolist() == [[1, 0, 2, 3], [5, 3, -1, -1]]
    assert rp.tolist() == [[0, 2, 4, 6, 7], [7, 8, 8, 8, 8]] and c.tolist() == [1, 2, 0, 0, 2, 3, 1, 1]
    assert cnt.dtype == ids.dtype == c.dtype == np.int32 and off.dtype == rp.dtype == np.int64
    # the prefix property: the order cut to 3 keeps the rows restricted to positions < 3
    short = subgraph_ref.rows(V, row_ptr, col, order[:3])
    assert [r.tolist() for r in short] == [r[r < 3].tolist() for r in rows[:3]]


def test_subgraph_ref_equals_the_double_loop_on_a_random_multigraph():
    rng = np.random.default_rng(3)
    V, E = 60, 400
    src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
    assert np.any(src == dst) and len(np.unique(src * V + dst)) < E  # self loops and duplicates
    o = rng.permutation(E)  # (rows in no particular order)
    o = o[np.argsort(src[o], kind="stable")]
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))])
    perm = rng.permutation(V)[:45]
    fast = subgraph_ref.rows(V, row_ptr, dst[o], perm)
    slow = subgraph_ref.brute_rows(V, row_ptr, dst[o], perm)
    assert len(fast) == len(slow) == 45
    for a, b in zip(fast, slow):
        assert np.array_equal(a, b)
    assert any(np.any(np.diff(r) == 0) for r in fast) and any(j in r for j, r in enumerate(fast))
    assert sum(len(r) for r in fast) < E
