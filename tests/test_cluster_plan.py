"""CPU-side checks of the conductance sweep (dppr_cluster, dppr_group_cluster): declared in include/dppr.h with DPPR_CLUSTER_MAX,
exported by the library, listed in engine.EXPORTS, rejected without a handle with nothing written; the HIP-free plan
(dynamicppr_amd/csrc/dppr_cluster_plan.hpp) driven by tests/native/cluster_plan_test.cpp as a stand-alone program under the address
and undefined-behaviour sanitizers; and the numpy restatement (tests/cluster_ref.py) against a six-vertex multigraph counted by
hand, against a brute-force set count on a random multigraph, and on the planted partition of tests/test_cluster_gpu.py with the
exact fixed point. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import cluster_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_cluster", "dppr_group_cluster")
ALPHA = 0.15


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    assert re.search(r"^#define DPPR_CLUSTER_MAX DPPR_TOPK_MAX\b", code, re.M)
    assert re.search(r"^#define DPPR_TOPK_MAX 8192\b", code, re.M) and eng.CLUSTER_MAX == 8192
    fields = re.search(r"typedef struct \{(.*?)\} dppr_cluster_t;", code, re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", fields) == [("int32_t", "count"), ("int32_t", "best_size"), ("int64_t", "best_cut"),
                                                    ("int64_t", "best_vol"), ("double", "best_phi")]
    assert [(n, t) for n, t in eng.Cluster._fields_] == [("count", ctypes.c_int32), ("best_size", ctypes.c_int32),
                                                         ("best_cut", ctypes.c_int64), ("best_vol", ctypes.c_int64),
                                                         ("best_phi", ctypes.c_double)]
    assert ctypes.sizeof(eng.Cluster) == 32
    # the contract is stated where a caller reads it
    for phrase in ("with multiplicity", "a self loop never crosses", "min(vol[j], Ed - vol[j])", "one IEEE division",
                   "smallest j among equal", "dppr_graph_edges", "Convergence is NOT"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("cluster", "group_cluster"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    best = (eng.Cluster * 2)()
    for b in best:
        b.count, b.best_size, b.best_cut, b.best_vol, b.best_phi = 7, 7, 7, 7, 2.5
    ids = (ctypes.c_int32 * 8)(*([7] * 8))
    arrs = [(ctypes.c_int64 * 8)(*([7] * 8)) for _ in range(3)]
    A = ctypes.addressof
    for fn in (L.dppr_cluster, L.dppr_group_cluster):
        assert fn(None, 0, -1, 4, 0.0, 1, A(best), A(ids), A(arrs[0]), A(arrs[1]), A(arrs[2])) == -1
    assert all(b.as_dict() == dict(count=7, best_size=7, best_cut=7, best_vol=7, best_phi=2.5) for b in best)
    assert list(ids) == [7] * 8 and all(list(a) == [7] * 8 for a in arrs)


def test_cluster_plan(tmp_path):
    """dppr_cluster_plan.hpp: the argument check at its limits, the sizes, the block for every combination of NULLs, cluster_best."""
    exe = str(tmp_path / "cluster_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "cluster_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cluster_ref_on_a_graph_counted_by_hand():
    """Six vertices, ten stored edges: 0->1 twice, 1->0, 1->2, the self loop 2->2, 2->3, 3->0, 3->4, 4->5, 5->3. Order 1, 0, 2, 3.
        S = {1}:          vol 2, out {1->0, 1->2} = 2, in {0->1, 0->1} = 2
        S = {1, 0}:       vol 4, out {1->2} = 1,        in {3->0} = 1
        S = {1, 0, 2}:    vol 6, out {2->3} = 1,        in {3->0} = 1       (2->2 never crosses)
        S = {1, 0, 2, 3}: vol 8, out {3->4} = 1,        in {5->3} = 1
    den = 2, 4, 4, 2; phi = 1, 1/4, 1/4, 1/2: the first of the two equal minima wins."""
    V, Ed = 6, 10
    row_ptr = np.array([0, 2, 4, 6, 8, 9, 10])
    col = np.array([1, 1, 0, 2, 2, 3, 0, 4, 5, 3])
    order = [1, 0, 2, 3]
    co, ci, vol = cluster_ref.prefix_arrays(V, row_ptr, col, order)
    assert co.tolist() == [2, 1, 1, 1] and ci.tolist() == [2, 1, 1, 1] and vol.tolist() == [2, 4, 6, 8]
    assert [a.tolist() for a in cluster_ref.brute_arrays(V, row_ptr, col, order)] == [co.tolist(), ci.tolist(), vol.tolist()]
    assert cluster_ref.best(co, vol, Ed, 1) == dict(count=4, best_size=2, best_cut=1, best_vol=4, best_phi=0.25)
    assert cluster_ref.best(co, vol, Ed, 3) == dict(count=4, best_size=3, best_cut=1, best_vol=6, best_phi=0.25)
    assert cluster_ref.best(co, vol, Ed, 4) == dict(count=4, best_size=4, best_cut=1, best_vol=8, best_phi=0.5)
    # an order that ends at the whole graph: the last prefix has den 0 and is not eligible; a k larger than the order pads
    b, ids, co, ci, vol = cluster_ref.cluster(V, row_ptr, col, Ed, [3, 4, 5, 0, 1, 2], 8, 6)
    assert b == dict(count=6, best_size=0, best_cut=0, best_vol=0, best_phi=float("inf"))
    assert ids.tolist() == [3, 4, 5, 0, 1, 2, -1, -1] and co.tolist() == [2, 2, 1, 2, 1, 0, 0, 0] and ci.tolist() == [2, 2, 1, 2, 1, 0, 0, 0]
    assert vol.tolist() == [2, 3, 4, 6, 8, 10, 0, 0] and ids.dtype == np.int32 and co.dtype == ci.dtype == vol.dtype == np.int64


def test_cluster_ref_equals_the_set_count_on_a_random_multigraph():
    rng = np.random.default_rng(3)
    V, E = 60, 400
    src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
    assert np.any(src == dst) and len(np.unique(src * V + dst)) < E  # self loops and duplicates
    order = np.lexsort((dst, src))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))])
    perm = rng.permutation(V)[:45]
    fast = cluster_ref.prefix_arrays(V, row_ptr, dst[order], perm)
    slow = cluster_ref.brute_arrays(V, row_ptr, dst[order], perm)
    for a, b in zip(fast, slow):
        assert np.array_equal(a, b)
    assert np.any(fast[0] != fast[1])


def planted_partition():
    """Blocks of 40 and 60 vertices, pair probability 0.3 drawn in (u, w > u) order per block from default_rng(5), and the bridges
    (b, 40 + b) for b = 0, 1, 2: the undirected edges (u, w) of the window that tests/test_cluster_gpu.py loads."""
    rng = np.random.default_rng(5)
    edges = []
    for lo, size in ((0, 40), (40, 60)):
        for u in range(lo, lo + size):
            for w in range(u + 1, lo + size):
                if rng.random() < 0.3:
                    edges.append((u, w))
    edges += [(b, 40 + b) for b in range(3)]
    return 100, np.array(edges, dtype=np.int32)


def test_the_planted_partition_is_found_by_the_exact_fixed_point():
    """With the fixed point of the `+ 1` recurrence for sources 5, 0 and 39, the order by p walks block A first -- the gap in p across
    the boundary is above 8e-4 -- and the best prefix is exactly vertices 0 .. 39: cut 3, vol 489, phi the double 3 / 489; the
    runner-up is at 0.0207 or above."""
    V, und = planted_partition()
    src, dst = np.concatenate([und[:, 0], und[:, 1]]), np.concatenate([und[:, 1], und[:, 0]])
    Ed = len(src)
    o = np.lexsort((dst, src))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))])
    outdeg = np.diff(row_ptr)
    A = np.zeros((V, V))
    np.add.at(A, (src, dst), 1.0)
    A = (1.0 - ALPHA) * A / (outdeg + 1.0)[:, None]
    for s in (5, 0, 39):
        b = np.zeros(V)
        b[s] = ALPHA
        p = np.linalg.solve(np.eye(V) - A, b)
        order = np.lexsort((np.arange(V), -p))
        assert sorted(order[:40].tolist()) == list(range(40)), s
        assert p[order[39]] - p[order[40]] > 8e-4, (s, p[order[39]] - p[order[40]])
        co, ci, vol = cluster_ref.prefix_arrays(V, row_ptr, dst[o], order)
        assert np.array_equal(co, ci)
        best = cluster_ref.best(co, vol, Ed, 1)
        assert best == dict(count=V, best_size=40, best_cut=3, best_vol=489, best_phi=3.0 / 489.0), (s, best)
        den = np.minimum(vol, Ed - vol)
        phi = np.where(den > 0, co / np.maximum(den, 1), np.inf)
        phi[39] = np.inf
        assert phi.min() >= 0.0207, (s, phi.min())
