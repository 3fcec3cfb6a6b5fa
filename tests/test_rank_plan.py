"""CPU-side checks of the ranked queries (dppr_topk_ranked, dppr_group_topk_ranked, dppr_rank_score_at, dppr_group_rank_score_at,
dppr_debug_rank_piece): declared in include/dppr.h with their contract, exported by the library, listed in engine.EXPORTS, rejected
without a handle; the HIP-free plan (dynamicppr_amd/csrc/dppr_rank_plan.hpp) driven by tests/native/rank_plan_test.cpp as a
stand-alone program under the address and undefined-behaviour sanitizers; the flags of ./pagerank; and the numpy reference
(tests/rank_ref.py) on a 6-vertex case worked out by hand. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_topk_ranked", "dppr_group_topk_ranked", "dppr_rank_score_at", "dppr_group_rank_score_at", "dppr_debug_rank_piece")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, value in (("DPPR_FACTOR_NONE", "0"), ("DPPR_FACTOR_DEV", "1"), ("DPPR_FACTOR_DEG", "2"), ("DPPR_FACTOR_INV_DEG", "3"),
                        ("DPPR_MASK_NONE", "0"), ("DPPR_MASK_ALLOW", "1"), ("DPPR_MASK_DENY", "2"), ("DPPR_EXCLUDE_SEEDS", "1u"),
                        ("DPPR_EXCLUDE_IN_NEIGHBOURS", "2u"), ("DPPR_EXCLUDE_OUT_NEIGHBOURS", "4u")):
        assert re.search(r"^#define " + name + r"\s+" + value + r"\b", code, re.M), name
    assert "dppr_rank_spec_t" in code
    assert (eng.FACTOR_NONE, eng.FACTOR_DEV, eng.FACTOR_DEG, eng.FACTOR_INV_DEG) == (0, 1, 2, 3)
    assert (eng.MASK_NONE, eng.MASK_ALLOW, eng.MASK_DENY) == (0, 1, 2)
    assert (eng.EXCLUDE_SEEDS, eng.EXCLUDE_IN_NEIGHBOURS, eng.EXCLUDE_OUT_NEIGHBOURS) == (1, 2, 4)
    # the contract is stated where a caller reads it
    for phrase in ("ONE rounding", "nothing fused", "scores exactly +0.0", "IN THAT LANE", "mean the same set", "Self loops and duplicate edges",
                   "follows the formula from p = 0.0", "+inf orders first", "bit for bit", "does not look at", "epoch rule of dppr_cluster",
                   "m == 0 is a valid no-op", "obtained before the first kernel", "OUT OF SCOPE", "0 for a parked vertex"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("topk_ranked", "group_topk_ranked", "rank_score_at", "group_rank_score_at", "debug_rank_piece", "rank_spec"):
        assert callable(getattr(eng.Engine, name)), name
    # the binding's struct is the header's: two ints, a pointer, an int, a pointer, an unsigned
    assert ctypes.sizeof(eng.RankSpec) == 40 and eng.RankSpec.factor_dev.offset == 8 and eng.RankSpec.mask.offset == 16
    assert eng.RankSpec.mask_dev.offset == 24 and eng.RankSpec.exclude.offset == 32
    s = eng.Engine.rank_spec(eng.FACTOR_DEV, 4096, eng.F32, eng.MASK_DENY, 8192, 5)
    assert (s.factor, s.factor_dtype, s.factor_dev, s.mask, s.mask_dev, s.exclude) == (1, 1, 4096, 2, 8192, 5)


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    ids, sc, cnt = np.full(4, 7, dtype=np.int32), np.full(4, 2.5), np.full(1, 7, dtype=np.int32)
    at = np.array([0, 1], dtype=np.int32)
    I, S, N, A = ids.ctypes.data_as(ip), sc.ctypes.data_as(dp), cnt.ctypes.data_as(ip), at.ctypes.data_as(ip)
    assert L.dppr_topk_ranked(None, 0, -1, None, 4, 0.0, I, S, N) == -1
    assert L.dppr_group_topk_ranked(None, 0, -1, None, 4, 0.0, I, S, N) == -1
    assert L.dppr_rank_score_at(None, 0, -1, None, A, 2, S) == -1
    assert L.dppr_group_rank_score_at(None, 0, -1, None, A, 2, S) == -1
    assert L.dppr_debug_rank_piece(None, 64) == -1
    assert np.all(ids == 7) and np.all(sc == 2.5) and np.all(cnt == 7)


def test_rank_plan(tmp_path):
    """dppr_rank_plan.hpp: every rejection at its limit, the flat seed list, the piece list against a brute-force split, its bound."""
    exe = str(tmp_path / "rank_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "rank_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cli_rank_arguments(tmp_path):
    """--rank-factor / --rank-exclude without --topk, with a value that is none of theirs, an empty token, or --split: invalid
    arguments and the usage, before any device work."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2"]
    for bad in (["--rank-factor", "deg"], ["--rank-exclude", "seeds"], ["--topk", "3", "--rank-factor", "degree"],
                ["--topk", "3", "--rank-factor", "DEG"], ["--topk", "3", "--rank-exclude", "seeds,both"],
                ["--topk", "3", "--rank-exclude", "seeds,,in"], ["--topk", "3", "--rank-exclude", ""],
                ["--topk", "3", "--rank-factor", "inv-deg", "--rank-exclude", "in,out,"],
                ["--topk", "3", "--rank-factor", "deg", "--split"]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--rank-factor <none|deg|inv-deg>" in r.stdout, (bad, r.stdout[-400:])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_reference_on_a_hand_computed_case():
    """Six vertices; stored edges 0->1 (twice), 0->2, 1->0, 2->4, 3->0, 4->4; vertex 5 has none. Lane 0 is the source 0, lane 1 the
    set {2, 4}. Every number below was worked out by hand from the definitions of include/dppr.h."""
    row = np.array([0, 3, 4, 5, 6, 7, 7])
    col = np.array([1, 1, 2, 0, 4, 0, 4])
    V = 6
    tails, heads = rank_ref.edges(row, col)
    assert tails.tolist() == [0, 0, 0, 1, 2, 3, 4] and heads.tolist() == col.tolist()
    deg = rank_ref.out_degree(V, tails)
    assert deg.tolist() == [3, 1, 1, 1, 1, 0]
    seeds = [[0], [2, 4]]

    def who(flags):
        return [np.nonzero(x)[0].tolist() for x in rank_ref.excluded(V, tails, heads, seeds, flags)]

    assert who(0) == [[], []]
    assert who(rank_ref.SEEDS) == [[0], [2, 4]]
    assert who(rank_ref.IN_NEIGHBOURS) == [[1, 3], [0, 2, 4]]   # (4 -> 4: the seed is its own neighbour)
    assert who(rank_ref.OUT_NEIGHBOURS) == [[1, 2], [4]]
    assert who(7) == [[0, 1, 2, 3], [0, 2, 4]]
    cols = [np.array([0.5, 0.25, 0.125, 0.0625, 0.03125, 0.0]), np.array([0.1, 0.0, 0.3, 0.2, 0.4, 0.05])]
    s = rank_ref.scores(cols, rank_ref.DEG, outdeg=deg)
    assert s[0].tolist() == [2.0, 0.5, 0.25, 0.125, 0.0625, 0.0]
    assert np.array_equal(bits(s[1]), bits(cols[1] * np.array([4.0, 2.0, 2.0, 2.0, 2.0, 1.0])))
    s = rank_ref.scores(cols, rank_ref.INV_DEG, outdeg=deg)
    assert s[0].tolist() == [0.125, 0.125, 0.0625, 0.03125, 0.015625, 0.0]
    ids, sc = rank_ref.topk(s[0], 5)
    assert ids.tolist() == [0, 1, 2, 3, 4] and ids.dtype == np.int32   # (the tie of 0 and 1 is cut by id; 5 scores 0 and never qualifies)
    assert rank_ref.topk(s[0], 1)[0].tolist() == [0] and rank_ref.topk(s[0], 5, 0.0625)[0].tolist() == [0, 1]
    # exclusion is per lane: 0 is excluded for lane 1 only, 3 for lane 0 only
    ex = rank_ref.excluded(V, tails, heads, seeds, rank_ref.SEEDS | rank_ref.IN_NEIGHBOURS)
    s = rank_ref.scores(cols, rank_ref.DEG, outdeg=deg, excl=ex)
    assert s[0].tolist() == [0.0, 0.0, 0.25, 0.0, 0.0625, 0.0] and rank_ref.topk(s[0], 8)[0].tolist() == [2, 4]
    assert rank_ref.topk(s[1], 8)[0].tolist() == [3, 5] and s[1][3] == 0.4 and s[1][5] == 0.05 and s[1][1] == 0.0
    # masks: deny {1}, allow {0, 2, 5}; a masked entry is +0.0
    s = rank_ref.scores(cols, deny=np.array([0, 1, 0, 0, 0, 0], dtype=np.uint8))
    assert rank_ref.topk(s[0], 8)[0].tolist() == [0, 2, 3, 4] and not np.signbit(s[0][1])
    s = rank_ref.scores(cols, allow=np.array([1, 0, 1, 0, 0, 1], dtype=bool))
    assert rank_ref.topk(s[0], 8)[0].tolist() == [0, 2] and rank_ref.topk(s[1], 8)[0].tolist() == [2, 0, 5]
    # a factor vector: zero, negative, +inf, NaN -- one product each; -x, 0 and NaN never qualify, +inf orders first
    g = np.array([0.0, -1.0, np.inf, np.nan, 2.0, 3.0], dtype=np.float32)
    s = rank_ref.scores(cols, rank_ref.DEV, g=g)
    assert s[0][0] == 0.0 and s[0][1] == -0.25 and s[0][2] == np.inf and np.isnan(s[0][3]) and s[0][4] == 0.0625
    assert s[0][5] == 0.0 and rank_ref.topk(s[0], 8)[0].tolist() == [2, 4]
    assert np.signbit(s[1][1]) and s[1][1] == 0.0 and rank_ref.topk(s[1], 8)[0].tolist() == [2, 4, 5]   # (0.0 * -1.0 is -0.0)
