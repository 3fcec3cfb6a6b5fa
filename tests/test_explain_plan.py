"""CPU-side checks of the explain queries (dppr_explain_at, dppr_group_explain_at, dppr_debug_explain): declared in include/dppr.h
with their contract, exported by the library, listed in engine.EXPORTS, rejected without a handle; the HIP-free plan
(dynamicppr_amd/csrc/dppr_explain_plan.hpp) driven by tests/native/explain_plan_test.cpp as a stand-alone program under the address
and undefined-behaviour sanitizers; the flags of ./pagerank; the numpy reference (tests/explain_ref.py) on cases worked by hand, and
on a state of the oracle: the decomposition identity and the monotone paths of a simple graph. No GPU call is made."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests import explain_ref as xr
from tests.util import small_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_explain_at", "dppr_group_explain_at", "dppr_debug_explain")
INV_TOL = 1e-13   # the project's tolerance of the invariant (tests/test_targets_gpu.py): the identity is the invariant summed in another order


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, val, mine in (("DPPR_EXPLAIN_MAX_M", 4096, eng.EXPLAIN_MAX_M), ("DPPR_EXPLAIN_MAX_F", 16, eng.EXPLAIN_MAX_F),
                            ("DPPR_EXPLAIN_MAX_DEPTH", 64, eng.EXPLAIN_MAX_DEPTH), ("DPPR_EXPLAIN_END_SEED", 0, eng.END_SEED),
                            ("DPPR_EXPLAIN_END_DEPTH", 1, eng.END_DEPTH), ("DPPR_EXPLAIN_END_DEAD", 2, eng.END_DEAD),
                            ("DPPR_EXPLAIN_END_CYCLE", 3, eng.END_CYCLE)):
        assert re.search(r"^#define " + name + r"\s+" + str(val) + r"\b", code, re.M) and mine == val, name
    assert (xr.END_SEED, xr.END_DEPTH, xr.END_DEAD, xr.END_CYCLE) == (0, 1, 2, 3)
    assert re.search(r"\}\s*dppr_explain_out_t;", code)
    # the contract is stated where a caller reads it
    for phrase in ("(((1.0 - 0.15) * p_i[w]) * (double)mult) / (double)(d(u) + 1)", "0x1.b333333333333p-1", "duplicates counted",
                   "A self loop is a head like any", "false for a NaN and for negatives", "c descending, external id of the head",
                   "self_i[u] = 0.15 * h_i[u]", "min(f, #heads with c > 0)", "-1 past the count", "path[j][i][0] = ids[j] always",
                   "DPPR_EXPLAIN_END_SEED (0)", "DPPR_EXPLAIN_END_DEPTH (1)", "DPPR_EXPLAIN_END_DEAD (2)", "DPPR_EXPLAIN_END_CYCLE (3)",
                   "u itself included: a self loop", "len[j][i] = t + 1", "path_c is 0.0 past len - 1", "0.0 past len",
                   "A duplicate id gives the same answer in each of its places", "Prefix property", "f + depth >= 1",
                   "m == 0 is valid and writes nothing", "Convergence is NOT required", "before any device work, nothing written",
                   "the id-map lock for the whole call", "output position comes from an atomic", "obtained before the first kernel",
                   "after DPPR_ERR_NOMEM", "dppr_debug_query_ms", "The results depend on neither", "OUT OF SCOPE"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("explain_at", "group_explain_at", "debug_explain"):
        assert callable(getattr(eng.Engine, name)), name
    assert ctypes.sizeof(eng.ExplainOut) == 12 * ctypes.sizeof(ctypes.c_void_p)


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip = ctypes.POINTER(ctypes.c_int32)
    guard = np.full(8, 7, dtype=np.int32)
    at = np.array([0, 1], dtype=np.int32)
    out = eng.ExplainOut()
    out.deg = out.len = out.path = guard.ctypes.data_as(ip)
    assert L.dppr_explain_at(None, 0, -1, at.ctypes.data_as(ip), 2, 1, 1, ctypes.byref(out)) == -1
    assert L.dppr_group_explain_at(None, 0, -1, at.ctypes.data_as(ip), 2, 1, 1, ctypes.byref(out)) == -1
    assert L.dppr_debug_explain(None, -1, 64) == -1
    assert np.all(guard == 7)


def test_explain_plan(tmp_path):
    """dppr_explain_plan.hpp: every rejection at its limit, the block layout of every combination of outputs (no overlap, doubles
    at multiples of 8, room only for what is asked), the memo decision, one wave per (query, lane)."""
    exe = str(tmp_path / "explain_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "explain_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cli_explain_arguments(tmp_path):
    """--explain with a missing file, a file without an id, a token that is no id, an id out of range, more than 4096 ids, F or D
    outside their limits, F + D == 0, the options without the flag, or --split: invalid arguments and the usage, before any device
    work."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    files = {"good": "0\n1\n\n2\n", "empty": "\n\n", "word": "0\nx\n", "negative": "0\n-1\n", "range": f"0\n{V}\n",
             "many": "\n".join(["1"] * 4097) + "\n"}
    for name, body in files.items():
        (tmp_path / name).write_text(body)
    good = str(tmp_path / "good")
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2"]
    for bad in (["--explain", str(tmp_path / "missing")], ["--explain", str(tmp_path / "empty")], ["--explain", str(tmp_path / "word")],
                ["--explain", str(tmp_path / "negative")], ["--explain", str(tmp_path / "range")], ["--explain", str(tmp_path / "many")],
                ["--explain", good, "--split"], ["--explain", good, "--explain-top", "17"], ["--explain", good, "--explain-top", "-1"],
                ["--explain", good, "--explain-depth", "65"], ["--explain", good, "--explain-depth", "-1"],
                ["--explain", good, "--explain-top", "0", "--explain-depth", "0"], ["--explain-top", "3"], ["--explain-depth", "3"]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--explain <file>" in r.stdout, (bad, r.stdout[-400:])


# ---- the reference on cases worked by hand ---------------------------------------------------------------------------------------
def fixed_point(V, tails, heads, source, sweeps=4000):
    """p of the exact fixed point of the invariant with r = 0, by Jacobi sweeps in numpy (a contraction by 0.85)."""
    deg = np.bincount(tails, minlength=V)
    p = np.zeros(V)
    for _ in range(sweeps):
        q = 0.85 * np.bincount(tails, weights=p[heads], minlength=V) / (deg + 1.0)
        q[source] += 0.15
        p = q
    return p


def test_reference_on_the_three_vertex_multigraph():
    """Edges 1->2 x5, 2->1 x5, 1->0, 2->0, seed 0. With q = p[1] = p[2]: p[0] = 0.15 (no out-edge), q = 0.85 (5 q + 0.15) / 7, so
    q = 0.1275 / 2.75 = 0.046363...; the best head of 1 is 2 (0.85 * q * 5 / 7 = 0.02815 against 0.85 * 0.15 / 7 = 0.01821) and of 2
    is 1: both paths turn back at their second vertex."""
    tails = np.array([1] * 5 + [2] * 5 + [1, 2])
    heads = np.array([2] * 5 + [1] * 5 + [0, 0])
    p = fixed_point(3, tails, heads, 0)
    assert abs(p[0] - 0.15) < 1e-15 and abs(p[1] - 0.1275 / 2.75) < 1e-15 and abs(p[2] - p[1]) < 1e-15
    g = xr.Graph(3, tails, heads)
    assert g.deg.tolist() == [0, 6, 6] and g.distinct.tolist() == [0, 2, 2]
    res = xr.explain(g, [p], [0], [0, 1, 2, 1], 4, 8)
    assert res["deg"].tolist() == [0, 6, 6, 6] and res["distinct"].tolist() == [0, 2, 2, 2]
    assert res["self"][:, 0].tolist() == [0.15, 0.0, 0.0, 0.0]
    assert res["nbr_count"][:, 0].tolist() == [0, 2, 2, 2]
    assert res["nbr"][1, 0].tolist() == [2, 0, -1, -1] and res["nbr_mult"][1, 0].tolist() == [5, 1, 0, 0]
    assert res["nbr"][2, 0].tolist() == [1, 0, -1, -1] and res["nbr_mult"][2, 0].tolist() == [5, 1, 0, 0]
    assert res["nbr_c"][1, 0, 0] == ((0.85 * p[2]) * 5.0) / 7.0 and res["nbr_c"][1, 0, 1] == ((0.85 * p[0]) * 1.0) / 7.0
    assert res["nbr_c"][1, 0, 2:].tolist() == [0.0, 0.0]
    assert res["end"][:, 0].tolist() == [xr.END_SEED, xr.END_CYCLE, xr.END_CYCLE, xr.END_CYCLE]
    assert res["len"][:, 0].tolist() == [1, 2, 2, 2]
    assert res["path"][1, 0].tolist() == [1, 2] + [-1] * 7 and res["path"][2, 0].tolist() == [2, 1] + [-1] * 7
    assert res["path_c"][1, 0, 0] == res["nbr_c"][1, 0, 0] and np.all(res["path_c"][1, 0, 1:] == 0.0)
    assert res["path_p"][1, 0, :2].tolist() == [p[1], p[2]] and np.all(res["path_p"][1, 0, 2:] == 0.0)
    for k in res:   # a duplicate id: the same answer in each of its places
        assert np.array_equal(res[k][1], res[k][3]), k
    # the decomposition identity, exact here up to rounding: p = self + sum of the contributions
    full = xr.explain(g, [p], [0], [0, 1, 2], 16, 0)
    assert np.max(np.abs(p - full["self"][:, 0] - full["nbr_c"][:, 0].sum(axis=1))) < 1e-16


def test_reference_on_the_chain():
    """15 -> 14 -> ... -> 0, seed 0: from 15 the seed is the 16th vertex of the path."""
    tails, heads = np.arange(15, 0, -1), np.arange(14, -1, -1)
    p = fixed_point(16, tails, heads, 0)
    assert p[0] == 0.15 and p[15] > 0
    g = xr.Graph(16, tails, heads)
    for depth, end, length in ((15, xr.END_SEED, 16), (64, xr.END_SEED, 16), (14, xr.END_DEPTH, 15)):
        res = xr.explain(g, [p], [0], [15], 1, depth)
        assert res["end"][0, 0] == end and res["len"][0, 0] == length, depth
        assert res["path"][0, 0, :length].tolist() == list(range(15, 15 - length, -1)) and np.all(res["path"][0, 0, length:] == -1)
        assert np.all(res["path_c"][0, 0, :length - 1] > 0) and np.all(res["path_c"][0, 0, length - 1:] == 0.0)
    res = xr.explain(g, [p], [0], [15, 0], 1, 0)   # depth 0: the vertex alone
    assert res["end"][:, 0].tolist() == [xr.END_DEPTH, xr.END_SEED] and res["len"][:, 0].tolist() == [1, 1] and res["path_c"].shape == (2, 1, 0)
    res = xr.explain(g, [p], [0], [15], 0, 1)      # f 0: no contributor is listed
    assert res["nbr"].shape == (1, 1, 0) and res["nbr_count"][0, 0] == 0 and res["len"][0, 0] == 2


def test_reference_on_a_self_loop():
    """1 -> 1 x3, 1 -> 0, 2 -> 1, seed 0: p[1] = 0.85 (3 p[1] + 0.15) / 5, so 3 p[1] = 0.156 > 0.15 and the best head of 1 is its own
    loop: the path of 1 ends at once as a cycle, the path of 2 after one hop; vertex 3 has no edge."""
    tails, heads = np.array([1, 1, 1, 1, 2]), np.array([1, 1, 1, 0, 1])
    p = fixed_point(4, tails, heads, 0)
    assert 3 * p[1] > p[0]
    g = xr.Graph(4, tails, heads)
    res = xr.explain(g, [p], [0], [1, 2, 3], 2, 5)
    assert res["nbr"][0, 0].tolist() == [1, 0] and res["nbr_mult"][0, 0].tolist() == [3, 1]
    assert res["end"][:, 0].tolist() == [xr.END_CYCLE, xr.END_CYCLE, xr.END_DEAD] and res["len"][:, 0].tolist() == [1, 2, 1]
    assert res["path"][1, 0, :2].tolist() == [2, 1] and res["deg"].tolist() == [4, 1, 0] and res["distinct"].tolist() == [2, 1, 0]


def test_reference_set_lane_and_the_order_of_ties():
    """A set lane: self = 0.15 * weight, a path ends at ANY seed of the set; heads of equal contribution are cut by id."""
    tails, heads = np.array([5, 5, 5, 4, 3]), np.array([3, 2, 4, 2, 2])
    p = np.array([0.0, 0.0, 0.5, 0.25, 0.25, 0.1])   # (any state: the order is defined for every p)
    g = xr.Graph(6, tails, heads)
    res = xr.explain(g, [p], [[(4, 0.3), (2, 0.7)]], [5, 4, 2, 0], 3, 4)
    assert res["self"][:, 0].tolist() == [0.0, 0.15 * 0.3, 0.15 * 0.7, 0.0]
    assert res["nbr"][0, 0].tolist() == [2, 3, 4]                       # 0.5 first, then the tie of 3 and 4 by id
    assert res["end"][:, 0].tolist() == [xr.END_SEED, xr.END_SEED, xr.END_SEED, xr.END_DEAD]
    assert res["path"][0, 0, :2].tolist() == [5, 2] and res["len"][:, 0].tolist() == [2, 1, 1, 1]
    nan = xr.explain(g, [np.array([0.0, 0.0, np.nan, -1.0, 0.25, 0.1])], [None], [5], 3, 1)
    assert nan["nbr"][0, 0].tolist() == [4, -1, -1] and nan["nbr_count"][0, 0] == 1   # a NaN and a negative never contribute


# ---- the identity and the monotone paths on a state of the oracle ----------------------------------------------------------------
def unique_window(directed, W=600):
    """The first W distinct edges of small_stream() without self loops (undirected: distinct as unordered pairs), then the rest of the
    stream: a window that is a simple graph."""
    V, e1, e2 = small_stream()
    keep, seen = [], set()
    for j, (a, b) in enumerate(zip(e1.tolist(), e2.tolist())):
        key = (a, b) if directed else (min(a, b), max(a, b))
        if a != b and key not in seen:
            seen.add(key)
            keep.append(j)
    keep = np.array(keep)
    assert len(keep) >= W + 100
    return V, e1[keep].astype(np.int32), e2[keep].astype(np.int32)


@pytest.mark.parametrize("directed", [1, 0])
def test_identity_and_monotone_paths_on_an_oracle_state(directed):
    from dynamicppr_amd import datagen
    from tests.util import window_directed_edges
    W, c, eps = 600, 20, 1e-9
    V, e1, e2 = unique_window(directed, W)
    src = int(datagen.top_sources(V, e1, e2, W, directed, 1)[0])
    og = orc.Graph(V, e1, e2, directed, W, c)
    s = orc.State(V, src, eps)
    s.sync_execute(og)
    p, r = np.array(s.p), np.array(s.r)
    tails, heads = window_directed_edges(og)
    g = xr.Graph(V, tails, heads)
    assert np.all(g.mult == 1) and np.all(g.tail != g.head)
    ids = np.arange(V)
    res = xr.explain(g, [p], [src], ids, 0, 64)
    # the decomposition: every contribution of every vertex (f is capped at 16 per call: the identity takes the whole order)
    total = np.zeros(V)
    for u in range(V):
        total[u] = xr.contributors(g, p, u)[2].sum()
    err = np.max(np.abs(p + xr.ALPHA * r - xr.ALPHA * xr.seed_vector(V, src) - total))
    print(f"directed={directed}: identity max err {err:.3e}")
    assert err <= INV_TOL
    starts = np.nonzero(p > 1e-4)[0]
    assert len(starts) > 100
    bound = math.ceil(math.log(1e4) / math.log(1.176)) + 1
    longest = 0
    for u in starts:
        n = int(res["len"][u, 0])
        assert res["end"][u, 0] == xr.END_SEED and n <= bound and res["path"][u, 0, n - 1] == src, u
        assert np.all(np.diff(res["path_p"][u, 0, :n]) > 0), u
        longest = max(longest, n)
    print(f"directed={directed}: {len(starts)} starts end at the seed, the longest path has {longest} vertices")
