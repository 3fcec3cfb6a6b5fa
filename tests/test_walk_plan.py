"""CPU-side checks of the forward walks (dppr_walks, dppr_refine_at, dppr_group_refine_at, dppr_debug_id_map): declared in
include/dppr.h with their limits, exported by the library, listed in engine.EXPORTS, rejected without a handle with nothing written;
the HIP-free plan and definition of a walk (dynamicppr_amd/csrc/dppr_walk_plan.hpp) driven by tests/native/walk_plan_test.cpp as a
stand-alone program under the address and undefined-behaviour sanitizers; the numpy restatement (tests/walk_ref.py) against the
same Philox known answers; and the rule itself: on a small multigraph, p + the mean residual at the endpoints lies within
Hoeffding's bound of the fixed point. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import walk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_walks", "dppr_refine_at", "dppr_group_refine_at", "dppr_debug_id_map")
ALPHA = 0.15


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    assert re.search(r"^#define DPPR_WALK_MAX_M 4096\b", code, re.M)
    assert re.search(r"^#define DPPR_WALK_MAX_W \(1 << 20\)", code, re.M)
    assert (eng.WALK_MAX_M, eng.WALK_MAX_W, eng.WALK_MAX_TOTAL) == (4096, 1 << 20, 1 << 26)
    # the contract is stated where a caller reads it: the generator, the threshold, the row order, the bias
    for phrase in ("Philox4x32-10", "0x26666666", "ascending INTERNAL id", "renumbering", "1e-8"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("walks", "walks_dev", "refine_at", "group_refine_at", "id_map"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ids = (ctypes.c_int32 * 2)(0, 1)
    ends = (ctypes.c_int32 * 8)(*([7] * 8))
    est, corr, sq = ((ctypes.c_double * 2)(2.5, 2.5) for _ in range(3))
    A = ctypes.addressof
    assert L.dppr_walks(None, -1, ids, 2, 4, 0, eng.DEST_HOST, A(ends)) == -1
    for fn in (L.dppr_refine_at, L.dppr_group_refine_at):
        assert fn(None, 0, -1, ids, 2, 4, 0, A(est), A(corr), A(sq)) == -1
    assert L.dppr_debug_id_map(None, ids) == -1
    assert list(ends) == [7] * 8 and list(ids) == [0, 1]
    assert list(est) == list(corr) == list(sq) == [2.5, 2.5]


def test_walk_plan(tmp_path):
    """dppr_walk_plan.hpp: the three Philox known answers; the pick at d = 0, d = 2^31 - 2 and x1:x2 = 0 / 2^64 - 1; the stop
    threshold at 0x26666665 / 0x26666666; the whole walk against a step-by-step restatement on rows of exactly their length; the
    waves' ranges covering every index once for m * W in {1, 63, 64, 65, .., 2^26}; sizes and argument checks."""
    exe = str(tmp_path / "walk_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "walk_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_walk_ref_passes_the_philox_known_answers():
    ones = 0xFFFFFFFF
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                           ((ones,) * 4, (ones, ones), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
                            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = tuple(int(x[0]) for x in walk_ref.philox(*ctr, *key))
        assert got == want, [hex(x) for x in got]
    # the pick at its edges, against Python's integers
    for x1, x2, d in ((0, 0, 0), (ones, ones, 0), (0, 0, 2**31 - 2), (ones, ones, 2**31 - 2), (0x80000000, 0, 1), (0x7FFFFFFF, ones, 1),
                      (0x12345678, 0x9ABCDEF0, 12345)):
        got = int(walk_ref.pick(np.array([x1], np.uint64), np.array([x2], np.uint64), np.array([d]))[0])
        assert got == (((x1 << 32) | x2) * (d + 1)) >> 64, (x1, x2, d)
    assert walk_ref.STOP_BELOW == int(0.15 * 2**32)


def _multigraph(V, E, seed):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))])
    return src, dst, row_ptr


def _reverse_push(V, src, dst, row_ptr, s, eps):
    """Reverse push to |r| <= eps under the invariant p[u] + a r[u] = a [u == s] + (1 - a) / (outdeg(u) + 1) * sum p[out(u)]."""
    outdeg = np.diff(row_ptr)
    p, r = np.zeros(V), np.zeros(V)
    r[s] = 1.0
    while True:
        front = np.nonzero(np.abs(r) > eps)[0]
        if len(front) == 0:
            return p, r
        for u in front:
            ru, r[u] = r[u], 0.0
            p[u] += ALPHA * ru
            tails = src[dst == u]  # every edge x -> u, duplicates kept
            np.add.at(r, tails, (1.0 - ALPHA) * ru / (outdeg[tails] + 1.0))


def test_the_rule_is_the_right_one():
    """V = 200, 1200 random directed edges with duplicates, a numpy reverse push to 1e-3: the invariant holds, and for every
    queried vertex p[v] + mean_w r[X_w] is within R sqrt(2 ln(2 / delta) / W) + 1e-8 R of the solution of the `+ 1` fixed point."""
    V, E, s, eps, W = 200, 1200, 7, 1e-3, 1 << 12
    src, dst, row_ptr = _multigraph(V, E, 5)
    assert len(np.unique(src * V + dst)) < E  # duplicates
    outdeg = np.diff(row_ptr)
    p, r = _reverse_push(V, src, dst, row_ptr, s, eps)
    A = np.zeros((V, V))
    np.add.at(A, (src, dst), 1.0)
    A = (1.0 - ALPHA) * A / (outdeg + 1.0)[:, None]
    b = np.zeros(V)
    b[s] = ALPHA
    assert np.max(np.abs(p + ALPHA * r - (b + A @ p))) < 1e-15
    pi = np.linalg.solve(np.eye(V) - A, b)
    R = float(np.max(np.abs(r)))
    assert 0 < R <= eps
    ident = np.arange(V)
    starts = np.arange(V)
    ends, steps = walk_ref.walks(row_ptr, dst, ident, ident, starts, W, seed=0x5EED, with_steps=True)
    t = walk_ref.terms(ends, [r])[0]
    est = p + t.mean(axis=1)
    bound = walk_ref.hoeffding(R, W)
    assert np.max(np.abs(est - pi)) <= bound, (np.max(np.abs(est - pi)), bound)
    assert np.max(np.abs(p - pi)) > bound  # the refinement is what brings it inside
    died = float(np.mean(ends < 0))
    assert 0.3 < died < 0.7 and 2.0 < steps.mean() < 1.0 / ALPHA, (died, steps.mean())  # (a walk may die before it would have stopped)
    # a walk is a function of (start, number, seed): another position in the call, another m, the same endpoints
    sub = np.array([150, 3, 150])
    again = walk_ref.walks(row_ptr, dst, ident, ident, sub, 100, seed=0x5EED)
    assert np.array_equal(again[0], ends[150, :100]) and np.array_equal(again[1], ends[3, :100]) and np.array_equal(again[0], again[2])
    assert not np.array_equal(walk_ref.walks(row_ptr, dst, ident, ident, sub, 100, seed=0x5EEE), again)


def gain_scenario():
    """The window of the test that shows the gain (tests/test_walks_gpu.py runs it on the engine): an R-MAT window of 2^10 vertex
    ids, 706 of them with an edge, two sources, solved to 1e-3; the queried vertices are the first source and the two vertices
    where plain p is worst for either source."""
    from dynamicppr_amd import datagen
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    W, c, directed = 4000, 50, 1
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 2)]
    return dict(V=V, e1=e1, e2=e2, W=W, c=c, directed=directed, sources=sources, eps=1e-3, queried=[sources[0], 744, 872],
                walks=1 << 16, seed=0x1234567890ABCDEF)


def test_the_gain_scenario_holds_for_the_restatement_alone():
    """Both halves of the GPU test on the CPU: the oracle's synchronous solve at 1e-3, walk_ref over the oracle's rows (numbered by
    external id), pi^ from the oracle's power iteration. Every refined value is inside Hoeffding's bound; plain p is outside it."""
    from oracle import oracle as orc
    sc = gain_scenario()
    V, Wk = sc["V"], sc["walks"]
    g = orc.Graph(V, sc["e1"], sc["e2"], sc["directed"], sc["W"], sc["c"])
    w1, w2 = g.window_edges()
    order = np.lexsort((w2, w1))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(w1, minlength=V))])
    ident = np.arange(V)
    ends = walk_ref.walks(row_ptr, w2[order], ident, ident, sc["queried"], Wk, sc["seed"])
    missed = 0
    for s in sc["sources"]:
        st = orc.State(V, s, sc["eps"])
        st.sync_execute(g)
        p, r = st.p.copy(), st.r.copy()
        pi, _ = orc.pow_rev(g, s)
        R = float(np.max(np.abs(r)))
        bound = walk_ref.hoeffding(R, Wk)
        est = p[sc["queried"]] + walk_ref.terms(ends, [r])[0].mean(axis=1)
        assert 0 < R <= sc["eps"] and np.all(np.abs(est - pi[sc["queried"]]) <= bound), (s, np.abs(est - pi[sc["queried"]]), bound)
        missed += int(np.sum(np.abs(p[sc["queried"]] - pi[sc["queried"]]) > bound))
    assert missed >= 1
