"""CPU-side checks of the forward sweep (dppr_forward, dppr_debug_forward): declared in include/dppr.h with their contract,
exported by the library, listed in engine.EXPORTS, rejected without a handle; the HIP-free plan
(dynamicppr_amd/csrc/dppr_forward_plan.hpp) driven by tests/native/forward_plan_test.cpp as a stand-alone program under the address
and undefined-behaviour sanitizers; the --forward flags of ./pagerank; the numpy reference (tests/forward_ref.py) on cases worked by
hand and against a dense solve. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import dot_ref
from tests import forward_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_forward", "dppr_debug_forward")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, val, mine in (("DPPR_FORWARD_MAX_M", 16, eng.FORWARD_MAX_M), ("DPPR_FORWARD_MAX_ITERS", 256, eng.FORWARD_MAX_ITERS),
                            ("DPPR_FORWARD_CHECK", 8, eng.FORWARD_CHECK), ("DPPR_FORWARD_AT_MAX", 4096, eng.FORWARD_AT_MAX)):
        assert re.search(r"^#define " + name + r"\s+" + str(val) + r"\b", code, re.M) and mine == val, name
    assert re.search(r"\}\s*dppr_forward_out_t;", code)
    for field in ("iters_used", "rem", "min_f", "topk_ids", "topk_f", "topk_counts", "at_ids", "n_at", "at_f", "dense_dev",
                  "dense_dtype", "dense_layout"):
        assert re.search(r"\b" + field + r"\s*[;,]", code), field
    # the contract is stated where a caller reads it
    for phrase in ("M[u][w] = 0.85 * mult(u -> w) / (d(u) + 1)", "the + 1 is death", "x_0 = e_q",
                   "f^K = 0.15 * sum_{k = 0 .. K} x_k", "0 <= pihat_q(t) - f^K[t] <= |x_{K+1}|_1 =: rem",
                   "numpy reproduces every output bit for bit", "y_k[u] = (0.85 * x_k[u]) / (double)(d(u) + 1)",
                   "once per vertex and", "THE FOLD of the dot family", "ascending internal tail id, duplicates as stored, self loops kept",
                   "blocks of\n *                    2^16 slots", "Every term is >= +0.0, so padding is exact",
                   "f[w] = f[w] + 0.15 * x_{k+1}[w]", "f starts as 0.15 * e_q", "holds +0.0",
                   "After the iterations 8, 16, 24, .. below iters and after iteration iters", "is FROZEN at that check",
                   "tol = 0 stops only a column whose mass has died out", "not of the other starts of the call",
                   "f = 0.15 * e_q, rem = 0.0, iters_used =\n *                    min(8, iters)", "a\n *                    renumbering may move last bits",
                   "a part whose pointers are all NULL is not run", "ties by external id ascending", "rounded once",
                   "before any device work, nothing written", "an epoch that is not resident", "reads back ONE word",
                   "nothing is read back between sweeps", "obtained\n * before the first kernel", "after DPPR_ERR_NOMEM",
                   "No output value comes from a floating-point atomic", "Every setting gives the same bits", "OUT OF SCOPE"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("forward", "debug_forward"):
        assert callable(getattr(eng.Engine, name)), name
    # the struct as the C compiler lays it out: 8 pointers, k and n_at padded to 8, min_f, the two enums
    assert ctypes.sizeof(eng.ForwardOut) == 96
    assert (eng.ForwardOut.k.offset, eng.ForwardOut.min_f.offset, eng.ForwardOut.topk_ids.offset) == (16, 24, 32)
    assert (eng.ForwardOut.at_ids.offset, eng.ForwardOut.n_at.offset, eng.ForwardOut.at_f.offset) == (56, 64, 72)
    assert (eng.ForwardOut.dense_dev.offset, eng.ForwardOut.dense_dtype.offset, eng.ForwardOut.dense_layout.offset) == (80, 88, 92)


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    guard, iguard = np.full(8, 7.0), np.full(8, 7, dtype=np.int32)
    starts = np.array([0, 1], dtype=np.int32)
    out = eng.ForwardOut()
    out.iters_used, out.rem = iguard.ctypes.data_as(ip), guard.ctypes.data_as(dp)
    assert L.dppr_forward(None, -1, starts.ctypes.data_as(ip), 2, 8, 0.0, ctypes.byref(out)) == -1
    assert L.dppr_debug_forward(None, 0, 0) == -1
    assert np.all(guard == 7.0) and np.all(iguard == 7)


def test_forward_plan(tmp_path):
    """dppr_forward_plan.hpp: every rejection at its limit, the parts of a call, the check schedule of every iters, the team and
    segment of every row width, the pieces of rows around every boundary, the bounds of the lists, and the row sum as the device
    forms it against the fold of the contract, bit for bit, for rows of 0 .. 131073 entries at five piece sizes."""
    exe = str(tmp_path / "forward_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "forward_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cli_forward_arguments(tmp_path):
    """--forward with a file that cannot be read or holds no id, options without the file, N / T / K outside their ranges, or
    --split: invalid arguments and the usage, before any device work."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    ids, empty, junk = tmp_path / "ids.txt", tmp_path / "empty.txt", tmp_path / "junk.txt"
    ids.write_text("1\n2\n3\n")
    empty.write_text("")
    junk.write_text("1\nx\n")
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2"]
    ok = ["--forward", str(ids)]
    for bad in (["--forward", str(tmp_path / "missing.txt")], ["--forward", str(empty)], ["--forward", str(junk)],
                ["--forward-iters", "8"], ["--forward-tol", "1e-3"], ["--forward-topk", "3"],
                ok + ["--forward-iters", "0"], ok + ["--forward-iters", "257"], ok + ["--forward-tol", "-1e-9"], ok + ["--forward-tol", "x"],
                ok + ["--forward-tol", "nan"], ok + ["--forward-tol", "inf"], ok + ["--forward-topk", "-1"], ok + ["--forward-topk", "65"],
                ok + ["--split"]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--forward <file>" in r.stdout, (bad, r.stdout[-400:])
        assert "forward " not in r.stdout.split("invalid arguments")[0], bad


# ---- the reference on cases worked by hand -----------------------------------------------------------------------------------------
def test_reference_on_a_chain_with_a_sink():
    """0 -> 1 -> 2, 2 a sink: d = (1, 1, 0). x_1 = 0.425 e_1, x_2 = 0.425^2 e_2, x_3 = 0: the column dies, and the first check sees it."""
    rows = fr.Rows.from_edges(3, [0, 1], [1, 2])
    f, rem, used = fr.forward(rows, 0, 64, 0.0)
    a = (0.85 * 1.0) / 2.0
    b = (0.85 * a) / 2.0
    assert used == 8 and rem == 0.0
    assert f.tolist() == [0.15, 0.15 * a, 0.15 * b]
    f1, rem1, used1 = fr.forward(rows, 0, 1, 0.0)
    assert used1 == 1 and rem1 == a and f1.tolist() == [0.15, 0.15 * a, 0.0]      # iteration iters stops every column, with the rem it has
    f2, rem2, used2 = fr.forward(rows, 0, 2, 1.0)
    assert used2 == 2 and rem2 == b
    # the sink as a start, and a vertex of no edge: f = 0.15 e_q, nothing remains, stopped at the first check
    for q in (2,):
        f, rem, used = fr.forward(rows, q, 64, 0.0)
        assert used == 8 and rem == 0.0 and f.tolist() == [0.0, 0.0, 0.15]
    assert fr.forward(rows, 2, 5, 0.0)[1:] == (0.0, 5)
    assert np.allclose(fr.forward(rows, 0, 64, 0.0)[0], fr.exact(3, [0, 1], [1, 2], 0), rtol=0, atol=1e-17)


def test_reference_on_a_self_loop():
    """0 -> 0 and 0 -> 1: d(0) = 2, the loop counts. x_k[0] = (0.85 / 3)^k, so f[0] = 0.15 / (1 - 0.85 / 3) in the limit."""
    rows = fr.Rows.from_edges(2, [0, 0], [0, 1])
    f, rem, used = fr.forward(rows, 0, 256, 0.0)
    g = 0.85 / 3.0
    assert abs(f[0] - 0.15 / (1.0 - g)) < 1e-15 and abs(f[1] - 0.15 * g / (1.0 - g)) < 1e-15
    f8, rem8, used8 = fr.forward(rows, 0, 8, 0.0)
    x = 1.0
    for _ in range(8):
        x = (0.85 * x) / 3.0
    assert used8 == 8 and rem8 == x + x        # x_8 = (x, x): the fold adds the two neighbours
    assert 0.0 <= f[0] - f8[0] <= rem8 and 0.0 <= f[1] - f8[1] <= rem8
    # tol: the first check at which rem <= tol, not the first iteration
    assert fr.forward(rows, 0, 64, rem8)[2] == 8 and fr.forward(rows, 0, 64, np.nextafter(rem8, 0))[2] == 16


def test_reference_on_a_duplicate_edge():
    """0 -> 1 twice and 0 -> 2: d(0) = 3, vertex 1 gets two terms -- added, as stored -- and twice what vertex 2 gets."""
    rows = fr.Rows.from_edges(3, [0, 0, 0], [1, 2, 1])
    f, rem, used = fr.forward(rows, 0, 64, 0.0)
    y = (0.85 * 1.0) / 4.0
    assert f.tolist() == [0.15, 0.15 * (y + y), 0.15 * y] and used == 8 and rem == 0.0
    once = fr.forward(fr.Rows.from_edges(3, [0, 0], [1, 2]), 0, 64, 0.0)[0]
    assert once[1] == once[2] == 0.15 * ((0.85 * 1.0) / 3.0)


def test_reference_orders_a_row_by_the_internal_id_of_the_tail():
    """The order of a row's terms is the device's: with the numbering reversed the last bits of a sum of three terms may move, and
    the reference follows the numbering it is given."""
    V = 5
    tails, heads = [0, 1, 2, 3, 3, 3], [3, 3, 3, 0, 1, 2]
    y = np.array([0.1, 0.7, 1e-17 + 0.3, 0.0, 0.0])
    up = fr.Rows.from_edges(V, tails, heads)
    down = fr.Rows.from_edges(V, tails, heads, ext2int=np.arange(V)[::-1].copy())
    assert up.tails[up.ptr[3]:up.ptr[4]].tolist() == [0, 1, 2] and down.tails[down.ptr[3]:down.ptr[4]].tolist() == [2, 1, 0]
    assert up.pull(y)[3] == (y[0] + y[1]) + (y[2] + 0.0) and down.pull(y)[3] == (y[2] + y[1]) + (y[0] + 0.0)


def test_reference_against_a_dense_solve():
    """50 vertices, 400 random edges with duplicates and self loops: 0 <= pihat - f <= rem entrywise at every K, to the rounding
    of the solve."""
    rng = np.random.default_rng(12)
    V = 50
    tails, heads = rng.integers(0, V, 400), rng.integers(0, V, 400)
    heads[:5] = tails[:5]
    rows = fr.Rows.from_edges(V, tails, heads)
    for q in (0, 17, 49):
        pi = fr.exact(V, tails, heads, q)
        for iters in (1, 5, 8, 30, 256):
            f, rem, used = fr.forward(rows, q, iters, 0.0)
            assert used == iters and rem > 0.0
            gap = pi - f
            assert np.all(gap >= -1e-15) and np.all(gap <= rem + 1e-15), (q, iters, gap.min(), gap.max(), rem)
        assert np.max(np.abs(pi - fr.forward(rows, q, 256, 0.0)[0])) < 1e-15
        # rem is the fold of x, and the sum of f grows towards the mass that dies: sum(pihat) = 0.15 * sum_k |x_k|_1
        f, rem, used = fr.forward(rows, q, 64, 1e-4)
        assert used % 8 == 0 and used < 64 and 0.0 < rem <= 1e-4
    # a column is a function of its start alone: the top k orders f descending, ties by id ascending
    f = fr.forward(rows, 0, 30, 0.0)[0]
    ids, fk = fr.topk(f, 10)
    assert ids[0] == 0 and np.all(np.diff(fk) <= 0) and len(ids) == 10
    tie = np.array([0.0, 0.5, 0.25, 0.5, 0.25])
    assert fr.topk(tie, 3)[0].tolist() == [1, 3, 2] and fr.topk(tie, 9, 0.25)[0].tolist() == [1, 3]
    assert dot_ref.fold(tie) == (0.0 + 0.5) + (0.25 + 0.5) + ((0.25 + 0.0) + 0.0)
