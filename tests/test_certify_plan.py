"""CPU-side checks of the certificate of a state (dppr_certify, dppr_group_certify, dppr_debug_certify): declared in include/dppr.h
with their contract, exported by the library, listed in engine.EXPORTS, rejected without a handle; the HIP-free plan
(dynamicppr_amd/csrc/dppr_certify_plan.hpp) driven by tests/native/certify_plan_test.cpp as a stand-alone program under the address
and undefined-behaviour sanitizers; the --certify flag of ./pagerank; the numpy reference (tests/certify_ref.py) on cases worked by
hand and on states of the oracle. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests import certify_ref as cr
from tests import dot_ref
from tests.test_explain_plan import fixed_point
from tests.util import invariant_max_err_np, small_stream, window_directed_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_certify", "dppr_group_certify", "dppr_debug_certify")
INV_TOL = 1e-13   # the project's tolerance of the invariant (tests/test_targets_gpu.py)


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, val, mine in (("DPPR_CERT_RESIDUAL", 1, eng.CERT_RESIDUAL), ("DPPR_CERT_INVARIANT", 2, eng.CERT_INVARIANT)):
        assert re.search(r"^#define " + name + r"\s+" + str(val) + r"\b", code, re.M) and mine == val, name
    assert re.search(r"\}\s*dppr_certify_out_t;", code)
    for field in ("max_abs_r", "argmax_r", "sum_abs_r", "sum_p", "n_pos", "n_neg", "n_nonfinite", "n_p_nonzero", "inv_max_err",
                  "inv_argmax", "state_epoch", "converged", "conv_eps"):
        assert re.search(r"\b" + field + r"\s*;", code), field
    # the contract is stated where a caller reads it
    for phrase in ("|p - p*|inf <= max_abs_r", "p - p* = M (p - p*) - alpha r", "in the live zone and the parked zone",
                   "A\n * vertex without an id has p = r = 0 and contributes nothing", "The inequalities are strict",
                   "r == eps is not counted", "Such a row counts here only", "0.0 with argmax_r[i] = -1",
                   "SMALLEST external id that attains it", "the fold of the dot family", "blocks of 2^16 slots",
                   "the slot of a vertex without an id holds +0.0", "dppr_dot_dense_dev returns for h = 1",
                   "numpy reproduces both sums bit for bit", "rows with p != 0",
                   "| (p_i[u] + 0.15 * r_i[u]) - (0.15 * h_i[u] + (0.85 * S_i[u]) / (double)(d(u) + 1)) |",
                   "duplicates count as stored, self loops count", "parked row has d = 0 and S = 0",
                   "smallest external id among the rows that attain the device's own", "is not part of the contract",
                   "return identical bits", "does NOT require that the state stands on `epoch`", "state_epoch tells which epoch",
                   "Convergence is not required", "before any device work, nothing written", "flags outside 1..3",
                   "a part all of whose pointers are NULL is simply not run", "the id-map lock for the whole call",
                   "with an explicit\n * epoch <= k", "obtained before the first kernel", "after DPPR_ERR_NOMEM", "dppr_debug_query_ms",
                   "do not depend on the grid size", "no output value comes from a floating-point atomic", "OUT OF SCOPE"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("certify", "group_certify", "debug_certify"):
        assert callable(getattr(eng.Engine, name)), name
    assert ctypes.sizeof(eng.CertifyOut) == 10 * ctypes.sizeof(ctypes.c_void_p) + 16
    assert eng.CertifyOut.state_epoch.offset == 80 and eng.CertifyOut.converged.offset == 84 and eng.CertifyOut.conv_eps.offset == 88


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    guard = np.full(8, 7.0)
    iguard = np.full(8, 7, dtype=np.int32)
    out = eng.CertifyOut()
    out.max_abs_r = out.inv_max_err = guard.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out.argmax_r = out.inv_argmax = iguard.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out.state_epoch, out.converged, out.conv_eps = 77, 77, 77.0
    assert L.dppr_certify(None, 0, -1, 1e-9, 3, ctypes.byref(out)) == -1
    assert L.dppr_group_certify(None, 0, -1, 1e-9, 3, ctypes.byref(out)) == -1
    assert L.dppr_debug_certify(None, 0, 0) == -1
    assert np.all(guard == 7.0) and np.all(iguard == 7)
    assert (out.state_epoch, out.converged, out.conv_eps) == (77, 77, 77.0)


def test_certify_plan(tmp_path):
    """dppr_certify_plan.hpp: every rejection at its limit, the block layout of every combination of outputs (no overlap, 8-byte
    planes at multiples of 8, room only for what is asked), the pieces of rows of 0, 1, piece - 1, piece, piece + 1 and 3 piece
    edges with every edge covered exactly once, the bound of the piece list."""
    exe = str(tmp_path / "certify_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "certify_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cli_certify_arguments(tmp_path):
    """--certify with N < 1, a token that is no whole number, or --split: invalid arguments and the usage, before any device work."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2"]
    for bad in (["--certify", "0"], ["--certify", "-1"], ["--certify", "x"], ["--certify", "2x"], ["--certify", "1.5"],
                ["--certify", ""], ["--certify", "1", "--split"]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--certify <N>" in r.stdout, (bad, r.stdout[-400:])
        assert "certify " not in r.stdout.split("invalid arguments")[0], bad


# ---- the reference on cases worked by hand ---------------------------------------------------------------------------------------
def test_reference_on_the_three_vertex_multigraph():
    """Edges 1->2 x5, 2->1 x5, 1->0, 2->0, seed 0, at its exact fixed point (r = 0): nothing is legal, every violation is rounding."""
    tails = np.array([1] * 5 + [2] * 5 + [1, 2])
    heads = np.array([2] * 5 + [1] * 5 + [0, 0])
    p = fixed_point(3, tails, heads, 0)
    res = cr.certify(3, tails, heads, [p], [np.zeros(3)], [0], 1e-9)
    assert res["n_pos"][0] == 0 and res["n_neg"][0] == 0 and res["n_nonfinite"][0] == 0 and res["n_p_nonzero"][0] == 3
    assert res["max_abs_r"][0] == 0.0 and res["argmax_r"][0] == 0 and res["sum_abs_r"][0] == 0.0   # (every row attains 0.0: the smallest id)
    assert res["sum_p"][0] == (p[0] + p[1]) + (p[2] + 0.0)                                         # the tree that adds neighbours
    assert np.all(res["err"] < 1e-15) and res["inv_max_err"][0] < 1e-15
    # the duplicates count as stored: with one copy of each edge the same p violates the invariant by a lot
    once = cr.invariant(3, np.array([1, 2, 1, 2]), np.array([2, 1, 0, 0]), [p], [np.zeros(3)], [0])
    assert once["inv_max_err"][0] > 1e-3


def test_reference_on_a_self_loop():
    """1 -> 1 x3, 1 -> 0, 2 -> 1, seed 0: the loop counts in d(1) = 4 and in S[1] = 3 p[1] + p[0]; vertex 3 has no edge (d = 0)."""
    tails, heads = np.array([1, 1, 1, 1, 2]), np.array([1, 1, 1, 0, 1])
    p = fixed_point(4, tails, heads, 0)
    assert abs(p[1] - 0.85 * (3 * p[1] + 0.15) / 5) < 1e-16 and p[3] == 0.0
    res = cr.certify(4, tails, heads, [p], [np.zeros(4)], [0], 1e-9)
    assert np.all(res["err"] < 1e-15) and res["n_p_nonzero"][0] == 3
    # a residual by hand: r[2] = 4e-9 moves the left side of row 2 alone by 0.15 * 4e-9
    r = np.array([0.0, 0.0, 4e-9, -2e-9])
    res = cr.certify(4, tails, heads, [p], [r], [0], 1e-9)
    assert (res["n_pos"][0], res["n_neg"][0]) == (1, 1) and res["max_abs_r"][0] == 4e-9 and res["argmax_r"][0] == 2
    assert res["sum_abs_r"][0] == (0.0 + 0.0) + (4e-9 + 2e-9)
    assert res["inv_argmax"][0] == 2 and abs(res["inv_max_err"][0] - 0.15 * 4e-9) < 1e-15   # (the fixed point's own 1e-15 above)
    # the inequalities are strict, ties go to the smaller id, a row that is not finite counts in n_nonfinite alone
    r = np.array([1e-9, -1e-9, np.nextafter(1e-9, 1), np.nextafter(1e-9, 1)])
    res = cr.residual([p], [r], 1e-9)
    assert (res["n_pos"][0], res["n_neg"][0]) == (2, 0) and res["argmax_r"][0] == 2
    res = cr.residual([np.array([np.nan, p[1], p[2], 0.0])], [np.array([0.5, 1e-3, np.inf, 0.0])], 1e-9)
    assert res["n_nonfinite"][0] == 2 and res["n_pos"][0] == 1 and res["max_abs_r"][0] == 1e-3 and res["argmax_r"][0] == 1
    assert res["sum_p"][0] == (0.0 + p[1]) + (0.0 + 0.0) and res["n_p_nonzero"][0] == 1
    none = cr.residual([np.zeros(2)], [np.zeros(2)], 1e-9, has_id=[False, False])
    assert none["max_abs_r"][0] == 0.0 and none["argmax_r"][0] == -1


def test_reference_on_a_set_lane_with_weights():
    """A set lane: h holds the weights. 2 -> 0, 2 -> 1 with seeds (0, 0.25), (1, 0.5): p[0] = 0.15 * 0.25, p[1] = 0.15 * 0.5,
    p[2] = 0.85 (p[0] + p[1]) / 3."""
    tails, heads = np.array([2, 2]), np.array([0, 1])
    seeds = [(0, 0.25), (1, 0.5)]
    p = np.array([0.15 * 0.25, 0.15 * 0.5, 0.85 * (0.15 * 0.25 + 0.15 * 0.5) / 3.0])
    res = cr.certify(3, tails, heads, [p], [np.zeros(3)], [seeds], 1e-9)
    assert res["inv_max_err"][0] < 1e-17
    wrong = cr.certify(3, tails, heads, [p], [np.zeros(3)], [[(0, 0.5), (1, 0.25)]], 1e-9)   # the weights swapped
    assert abs(wrong["inv_max_err"][0] - 0.15 * 0.25) < 1e-17 and wrong["inv_argmax"][0] == 0
    as_source = cr.certify(3, tails, heads, [p], [np.zeros(3)], [0], 1e-9)                     # read as the source lane of vertex 0
    assert abs(as_source["inv_max_err"][0] - 0.15 * 0.75) < 1e-17 and as_source["inv_argmax"][0] == 0


def test_reference_on_a_vertex_without_out_edges():
    """A parked-style vertex: no stored edge (d = 0, S = 0) but a state. The invariant asks p + 0.15 r = 0.15 h of it."""
    tails, heads = np.array([0]), np.array([1])
    p, r = np.array([0.0, 0.0, 0.3]), np.array([0.0, 0.0, -2.0])   # vertex 2: 0.3 + 0.15 * -2 = 0
    res = cr.certify(3, tails, heads, [p], [r], [None], 1e-9)
    assert res["inv_max_err"][0] < 1e-17 and res["n_neg"][0] == 1 and res["argmax_r"][0] == 2
    p[2] = 0.3 + 1e-6
    res = cr.certify(3, tails, heads, [p], [r], [None], 1e-9)
    assert res["inv_argmax"][0] == 2 and abs(res["inv_max_err"][0] - 1e-6) < 1e-15


def test_reference_two_lanes_and_the_fold():
    """Lanes are independent, and the sums are dot_ref.fold of the terms by external id (not the running sum)."""
    rng = np.random.default_rng(3)
    V = 70000   # more than one block of 2^16 slots
    p, r = [rng.random(V), rng.random(V)], [rng.standard_normal(V) * 1e-9, rng.standard_normal(V) * 1e-9]
    res = cr.residual(p, r, 1e-9)
    for i in range(2):
        one = cr.residual([p[i]], [r[i]], 1e-9)
        for k in res:
            assert res[k][i] == one[k][0], (k, i)
        assert res["sum_p"][i] == dot_ref.fold_stated(p[i]) and res["sum_abs_r"][i] == dot_ref.fold_stated(np.abs(r[i]))
        assert res["n_pos"][i] == int((r[i] > 1e-9).sum()) and res["n_neg"][i] == int((r[i] < -1e-9).sum())
    assert res["sum_p"][0] != dot_ref.running(p[0])


# ---- a state of the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_reference_on_an_oracle_state(directed):
    from dynamicppr_amd import datagen
    W, c, eps = 600, 20, 1e-9
    V, e1, e2 = small_stream()
    src = int(datagen.top_sources(V, e1, e2, W, directed, 1)[0])
    og = orc.Graph(V, e1, e2, directed, W, c)
    s = orc.State(V, src, eps)
    s.sync_execute(og)
    p, r = np.array(s.p), np.array(s.r)
    tails, heads = window_directed_edges(og)
    res = cr.certify(V, tails, heads, [p], [r], [src], eps)
    print(f"directed={directed}: max|r| {res['max_abs_r'][0]:.3e} inv {res['inv_max_err'][0]:.3e} nonzero {res['n_p_nonzero'][0]}")
    assert res["n_pos"][0] == 0 and res["n_neg"][0] == 0 and res["n_nonfinite"][0] == 0
    assert 0.0 < res["max_abs_r"][0] < eps and res["max_abs_r"][0] == np.max(np.abs(r))
    assert res["inv_max_err"][0] < INV_TOL
    assert abs(res["inv_max_err"][0] - invariant_max_err_np(p, r, tails, heads, V, src)) < 1e-16   # the suite's own evaluation
    assert res["n_p_nonzero"][0] == np.count_nonzero(p) > 100
    assert res["sum_p"][0] == dot_ref.fold(p) and abs(res["sum_p"][0] - p.sum()) < 1e-12
