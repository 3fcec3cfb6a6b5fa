"""CPU-side checks of the forward push (dppr_forward_push, dppr_debug_forward_push): declared in include/dppr.h with their contract,
exported by the library, listed in engine.EXPORTS, rejected without a handle; the HIP-free plan
(dynamicppr_amd/csrc/dppr_fpush_plan.hpp) driven by tests/native/fpush_plan_test.cpp as a stand-alone program under the address and
undefined-behaviour sanitizers, its host round held against tests/fpush_ref.py bit for bit on a hand-made graph; the --forward-push
flags of ./pagerank; the numpy reference on cases worked by hand and against a dense solve. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import forward_ref as fr
from tests import fpush_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_forward_push", "dppr_debug_forward_push")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, val, mine in (("DPPR_FPUSH_SET_MAX", 4096, eng.FPUSH_SET_MAX), ("DPPR_FPUSH_MAX_ROUNDS", 256, eng.FPUSH_MAX_ROUNDS)):
        assert re.search(r"^#define " + name + r"\s+" + str(val) + r"\b", code, re.M) and mine == val, name
    assert re.search(r"\}\s*dppr_forward_push_out_t;", code)
    for field in ("rounds_used", "converged", "rem", "pushes", "left", "work", "min_p", "topk_ids", "topk_p", "topk_counts", "at_ids",
                  "n_at", "at_p", "at_r", "dense_p_dev", "dense_r_dev", "dense_dtype", "dense_layout"):
        assert re.search(r"\b" + field + r"\s*[;,]", code), field
    for phrase in ("thr[u] = eps * (double)(d(u) + 1)", "F = { u : r[u] > thr[u] }, a strict comparison", "rounds_used = k - 1",
                   "p[u] = p[u] + 0.15 * r[u]", "r[u] = +0.0", "THE FOLD of the dot family", "r[w] keeps its bits",
                   "the device skips every row without a frontier in-neighbour", "The\n *                    definition stays the dense one",
                   "p[q] = 0.15 * w and r[q] = +0.0", "counts in no statistic", "not of the other columns",
                   "0 <= pihat_h[t] - p[t] <= rem entrywise", "r[u] <= eps * (d(u) + 1) everywhere", "error <= rem * max|r_reverse|",
                   "0 if and only if converged", "over the UNION of the columns' frontiers", "a part whose pointers are all NULL is not run",
                   "before any device work, nothing written", "then reads ONE word", "No output value comes from a floating-point atomic",
                   "the\n * order of the frontier and receiver lists enters no value", "Every setting gives the same bits", "OUT OF SCOPE"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("forward_push", "debug_forward_push"):
        assert callable(getattr(eng.Engine, name)), name
    # the struct as the C compiler lays it out: 6 pointers, k padded to 8, min_p, 4 pointers, n_at padded, 4 pointers, the two enums
    o = eng.ForwardPushOut
    assert ctypes.sizeof(o) == 144
    assert (o.work.offset, o.k.offset, o.min_p.offset, o.topk_ids.offset) == (40, 48, 56, 64)
    assert (o.at_ids.offset, o.n_at.offset, o.at_p.offset, o.at_r.offset) == (88, 96, 104, 112)
    assert (o.dense_p_dev.offset, o.dense_r_dev.offset, o.dense_dtype.offset, o.dense_layout.offset) == (120, 128, 136, 140)


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip, dp, lp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    guard, iguard = np.full(8, 7.0), np.full(8, 7, dtype=np.int32)
    off, ids, w = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.ones(2)
    out = eng.ForwardPushOut()
    out.rounds_used, out.rem = iguard.ctypes.data_as(ip), guard.ctypes.data_as(dp)
    assert L.dppr_forward_push(None, -1, off.ctypes.data_as(lp), ids.ctypes.data_as(ip), w.ctypes.data_as(dp), 2, 1e-6, 8, ctypes.byref(out)) == -1
    assert L.dppr_debug_forward_push(None, 0, 0, 0) == -1
    assert np.all(guard == 7.0) and np.all(iguard == 7)


# the hand-made graph of tests/native/fpush_plan_test.cpp, as stored edges tail -> head in the order of its in-CSR
TAILS, HEADS = [2, 3, 0, 0, 1, 1, 2], [0, 0, 1, 2, 2, 2, 2]
COLUMNS = (([0], [1.0], 1e-3), ([3, 1], [0.7, 2.5], 1e-2), ([2], [1e-4], 1e-3))


def test_fpush_plan_and_the_host_round_against_numpy(tmp_path):
    """dppr_fpush_plan.hpp: every rejection at its limit, the CSR checks, the parts of a call, every chunk schedule, the sizes, the
    top-k insertion -- and the host round, whose p, r and |F| after each of 12 rounds of three columns (alternating piece sizes) are
    the bits of tests/fpush_ref.py stopped after as many rounds."""
    exe = str(tmp_path / "fpush_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "fpush_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
    rows = fr.Rows.from_edges(5, TAILS, HEADS)
    assert rows.ptr.tolist() == [0, 2, 3, 7, 7, 7] and rows.tails.tolist() == TAILS and rows.d.tolist() == [2, 2, 2, 1, 0]
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("round ")]
    assert len(lines) == 3 * 12
    none = np.zeros(5, dtype=bool)   # (vertex 4 is no seed)
    for l in lines:
        c, k, n = int(l[1]), int(l[2]), int(l[3])
        ids, w, eps = COLUMNS[c]
        want = pr.push(rows, none, ids, w, eps, k)
        p = np.array([int(x, 16) for x in l[4::2]], dtype=np.uint64).view(np.float64)
        rr = np.array([int(x, 16) for x in l[5::2]], dtype=np.uint64).view(np.float64)
        assert np.array_equal(p.view(np.uint64), want.p.view(np.uint64)) and np.array_equal(rr.view(np.uint64), want.r.view(np.uint64)), (c, k)
        assert n == (int(want.fronts[k - 1].sum()) if k <= want.rounds_used else 0), (c, k)
    assert any(int(l[3]) > 0 for l in lines) and any(int(l[3]) == 0 for l in lines)


def test_cli_forward_push_arguments(tmp_path):
    """--forward-push with a file that cannot be read or holds no set, options without the file, a missing or bad --push-eps, N
    outside its range, or --split: invalid arguments and the usage, before any device work."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    sets, empty, junk = tmp_path / "sets.txt", tmp_path / "empty.txt", tmp_path / "junk.txt"
    sets.write_text("1\n2:0.5 3:2\n")
    empty.write_text("")
    junk.write_text("1\nx:1\n")
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2"]
    ok = ["--forward-push", str(sets), "--push-eps", "1e-5"]
    for bad in (["--forward-push", str(tmp_path / "missing.txt"), "--push-eps", "1e-5"], ["--forward-push", str(empty), "--push-eps", "1e-5"],
                ["--forward-push", str(junk), "--push-eps", "1e-5"], ["--push-eps", "1e-5"], ["--push-rounds", "8"],
                ["--forward-push", str(sets)], ok[:2] + ["--push-eps", "0"], ok[:2] + ["--push-eps", "-1e-9"], ok[:2] + ["--push-eps", "x"],
                ok[:2] + ["--push-eps", "nan"], ok[:2] + ["--push-eps", "inf"], ok + ["--push-rounds", "0"], ok + ["--push-rounds", "257"],
                ok + ["--forward-topk", "65"], ok + ["--split"]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--forward-push <file>" in r.stdout, (bad, r.stdout[-400:])
        assert "fpush " not in r.stdout.split("invalid arguments")[0], bad


# ---- the reference on cases worked by hand -----------------------------------------------------------------------------------------
def test_reference_on_a_chain_with_a_sink():
    """0 -> 1 -> 2, 2 a sink: d = (1, 1, 0). Each round pushes one vertex; the sink's push sends nothing on."""
    rows = fr.Rows.from_edges(3, [0, 1], [1, 2])
    c = pr.push(rows, pr.rowless_mask(rows), 0, 1.0, 1e-3, 64)
    assert c.rounds_used == 3 and c.converged == 1 and c.pushes == 3 and c.left == 0 and c.rem == 0.0
    assert c.p.tolist() == [0.15, 0.15 * 0.425, 0.15 * ((0.85 * 0.425) / 2.0)] and not c.r.any()
    assert pr.work(rows, [c]).tolist() == [3, 2, 2]   # the sink is pushed, but it has no head to gather
    # eps above the second vertex's share: it keeps its residual
    c = pr.push(rows, pr.rowless_mask(rows), 0, 1.0, 0.3, 64)
    assert c.rounds_used == 1 and c.converged == 1 and c.r.tolist() == [0.0, 0.425, 0.0] and c.rem == 0.425 and c.p.tolist() == [0.15, 0.0, 0.0]
    # the cap: stopped while a vertex is above thr
    c = pr.push(rows, pr.rowless_mask(rows), 0, 1.0, 1e-3, 1)
    assert c.rounds_used == 1 and c.converged == 0 and c.left == 1
    # exactly as many rounds as it needs: the comparison after the last round finds nothing
    c = pr.push(rows, pr.rowless_mask(rows), 0, 1.0, 1e-3, 3)
    assert c.rounds_used == 3 and c.converged == 1


def test_reference_settles_a_seed_without_a_row_and_keeps_the_strict_comparison():
    rows = fr.Rows.from_edges(4, [0, 1], [1, 0])   # 2 and 3 are named by no edge
    rowless = pr.rowless_mask(rows)
    assert rowless.tolist() == [False, False, True, True]
    c = pr.push(rows, rowless, [2, 0], [1e-9, 1.0], 1e-3, 64)   # far below eps, and settled all the same
    assert c.p[2] == 0.15 * 1e-9 and c.r[2] == 0.0 and c.pushes == c.rounds_used and c.fronts[0].tolist() == [True, False, False, False]
    alone = pr.push(rows, rowless, 0, 1.0, 1e-3, 64)
    assert np.array_equal(alone.p[:2], c.p[:2]) and np.array_equal(alone.r, c.r) and alone.rem == c.rem
    only = pr.push(rows, rowless, 3, 2.0, 1e-3, 64)
    assert only.rounds_used == 0 and only.converged == 1 and only.pushes == 0 and only.rem == 0.0 and only.p.tolist() == [0, 0, 0, 0.3]
    # r == thr is not pushed: d(0) = 1, thr = 2 eps
    at_thr = pr.push(rows, rowless, 0, 0.5, 0.25, 64)
    assert at_thr.rounds_used == 0 and at_thr.r[0] == 0.5 and at_thr.left == 0 and at_thr.converged == 1
    above = pr.push(rows, rowless, 0, np.nextafter(0.5, 1.0), 0.25, 1)
    assert above.rounds_used == 1


def test_reference_keeps_the_entrywise_bound_and_the_identity():
    """On random small graphs: 0 <= pihat_h - p <= rem, r <= thr once converged, and p + sum_u r[u] pihat_u = pihat_h."""
    rng = np.random.default_rng(9)
    for V, E in ((12, 40), (40, 90)):
        tails, heads = rng.integers(0, V, E), rng.integers(0, V, E)
        rows = fr.Rows.from_edges(V, tails, heads)
        rowless = pr.rowless_mask(rows)
        pi = np.stack([fr.exact(V, tails, heads, q) for q in range(V)])   # pi[q] = pihat_q
        ids = rng.choice(np.nonzero(~rowless)[0], 3, replace=False)
        w = rng.random(3) + 0.2
        exact = w @ pi[ids]
        for eps, cap in ((1e-2, 64), (1e-5, 64), (1e-7, 4)):
            c = pr.push(rows, rowless, ids, w, eps, cap)
            gap = exact - c.p
            assert np.all(gap >= -1e-14) and np.all(gap <= c.rem + 1e-14)
            assert np.max(np.abs(c.p + c.r @ pi - exact)) < 1e-14
            assert c.converged == int(np.all(c.r <= eps * (rows.d + 1.0)))
        assert pr.push(rows, rowless, ids, w, 1e-7, 4).converged == 0 and pr.push(rows, rowless, ids, w, 1e-2, 64).converged == 1
