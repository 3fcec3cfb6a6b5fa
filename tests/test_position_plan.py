"""CPU-side checks of the position queries (dppr_position_at, dppr_group_position_at, dppr_debug_position_tile): declared in
include/dppr.h with their contract, exported by the library, listed in engine.EXPORTS, rejected without a handle; the HIP-free plan
(dynamicppr_amd/csrc/dppr_position_plan.hpp) driven by tests/native/position_plan_test.cpp as a stand-alone program under the
address and undefined-behaviour sanitizers; the flags of ./pagerank; the numpy reference (tests/position_ref.py) on the 6-vertex
case of tests/test_rank_plan.py worked out by hand; and rank_metrics on a case worked by hand. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import position_ref, rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_position_at", "dppr_group_position_at", "dppr_debug_position_tile")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    assert re.search(r"^#define DPPR_POSITION_MAX\s+4096\b", code, re.M) and eng.POSITION_MAX == 4096
    # the contract is stated where a caller reads it
    for phrase in ("THE SCORE of dppr_topk_ranked for lane i, unchanged", "spec == NULL means the score", "iff score_i[v] > min_score",
                   "never qualifies, +inf does", "pos[j][i] = -1", "score_i[u] == score_i[v] and u < v", "0-based position",
                   "denominator of a percentile", "at unlimited k", "The live and the parked zone are both counted",
                   "never qualifies and never precedes", "A duplicate id gives the same answer in each of its places", "ANCHORS",
                   "returns ids[j] at", "0, 1, .., count - 1", "dppr_group_topk(k, min_p = min_score)", "m == 0 is valid",
                   "before any device work, nothing written", "m > DPPR_POSITION_MAX", "min_score negative or NaN",
                   "every spec and epoch rejection of dppr_topk_ranked", "the id-map lock for the whole call", "not a second one",
                   "12 m n bytes", "4 (m + 1) n bytes", "obtained before the first kernel", "after DPPR_ERR_NOMEM", "OUT OF SCOPE",
                   "The results do not depend on it"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("position_at", "group_position_at", "debug_position_tile"):
        assert callable(getattr(eng.Engine, name)), name
    assert callable(eng.rank_metrics)


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip = ctypes.POINTER(ctypes.c_int32)
    pos, cnt = np.full(4, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    at = np.array([0, 1], dtype=np.int32)
    P, N, A = pos.ctypes.data_as(ip), cnt.ctypes.data_as(ip), at.ctypes.data_as(ip)
    assert L.dppr_position_at(None, 0, -1, None, 0.0, A, 2, P, N) == -1
    assert L.dppr_group_position_at(None, 0, -1, None, 0.0, A, 2, P, N) == -1
    assert L.dppr_debug_position_tile(None, 64) == -1
    assert np.all(pos == 7) and np.all(cnt == 7)


def test_position_plan(tmp_path):
    """dppr_position_plan.hpp: every rejection at its limit, the workspace layout, the LDS budget of every (n, m, tile), lane blocks
    and passes that cover every (lane, query) exactly once against brute force."""
    exe = str(tmp_path / "position_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "position_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cli_position_arguments(tmp_path):
    """--positions with a missing file, a file without an id, a token that is no id, an id out of range, more than 4096 ids, or
    --split: invalid arguments and the usage, before any device work."""
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
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2"]
    for bad in (["--positions", str(tmp_path / "missing")], ["--positions", str(tmp_path / "empty")], ["--positions", str(tmp_path / "word")],
                ["--positions", str(tmp_path / "negative")], ["--positions", str(tmp_path / "range")], ["--positions", str(tmp_path / "many")],
                ["--positions", str(tmp_path / "good"), "--split"], ["--positions", str(tmp_path / "good"), "--rank-factor", "degree"],
                ["--positions", str(tmp_path / "good"), "--rank-exclude", "seeds,both"]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--positions <file>" in r.stdout, (bad, r.stdout[-400:])


def test_reference_on_a_hand_computed_case():
    """The six vertices of tests/test_rank_plan.py: stored edges 0->1 (twice), 0->2, 1->0, 2->4, 3->0, 4->4; vertex 5 has none.
    Out-degrees 3, 1, 1, 1, 1, 0. Every number below was worked out by hand from the definitions of include/dppr.h."""
    deg = np.array([3, 1, 1, 1, 1, 0])
    cols = [np.array([0.5, 0.25, 0.125, 0.0625, 0.03125, 0.0]), np.array([0.1, 0.0, 0.3, 0.2, 0.4, 0.05])]
    ids = np.arange(6)
    # INV_DEG, lane 0: 0.125, 0.125, 0.0625, 0.03125, 0.015625, 0 -- the tie of 0 and 1 is cut by id, 5 scores 0 and never qualifies
    s = position_ref.scores(cols, rank_ref.INV_DEG, outdeg=deg)
    pos, cnt = position_ref.positions(s[0], ids)
    assert pos.tolist() == [0, 1, 2, 3, 4, -1] and cnt == 5 and pos.dtype == np.int32
    assert position_ref.order(s[0]).tolist() == [0, 1, 2, 3, 4]
    pos, cnt = position_ref.positions(s[0], ids, 0.0625)   # (strictly above: 2 falls out with its 0.0625)
    assert pos.tolist() == [0, 1, -1, -1, -1, -1] and cnt == 2
    # lane 1: 0.025, 0, 0.15, 0.1, 0.2, 0.05 -> 4, 2, 3, 5, 0
    pos, cnt = position_ref.group_positions(s, [4, 0, 1, 4, 5])
    assert pos.tolist() == [[4, 0], [0, 4], [1, -1], [4, 0], [-1, 3]] and cnt.tolist() == [5, 5] and pos.dtype == np.int32
    # a factor vector of zero, negative, +inf, NaN: lane 0 is 0, -0.25, inf, nan, 0.0625, 0 -> 2 then 4, the rest never
    g = np.array([0.0, -1.0, np.inf, np.nan, 2.0, 3.0], dtype=np.float32)
    s = position_ref.scores(cols, rank_ref.DEV, g=g)
    pos, cnt = position_ref.positions(s[0], ids)
    assert pos.tolist() == [-1, -1, 0, -1, 1, -1] and cnt == 2
    # lane 1 is 0, -0, inf, nan, 0.8, 0.15 -> 2, 4, 5
    pos, cnt = position_ref.positions(s[1], ids)
    assert pos.tolist() == [-1, -1, 0, -1, 1, 2] and cnt == 3
    # no id, no lane
    pos, cnt = position_ref.group_positions(s, [])
    assert pos.shape == (0, 2) and cnt.tolist() == [2, 3]


def test_rank_metrics_on_a_hand_computed_case():
    """Positions 0, 2, -1, 9: reciprocal ranks 1, 1/3, 0, 1/10; hits below 1: one, below 3: two, below 10: three."""
    mrr, hits = eng.rank_metrics(np.array([0, 2, -1, 9], dtype=np.int32), (1, 3, 10))
    assert mrr == (1.0 + 1.0 / 3 + 1.0 / 10) / 4
    assert hits == {1: 0.25, 3: 0.5, 10: 0.75}
    assert eng.rank_metrics([], (5,)) == (0.0, {5: 0.0})
    assert eng.rank_metrics([-1, -1], (1,)) == (0.0, {1: 0.0})
    assert eng.rank_metrics([3], ())[0] == 0.25
