"""CPU-side checks of the ranked, position and sample queries over a forward track (dppr_ftrack_topk_ranked, dppr_ftrack_rank_score_at,
dppr_ftrack_position_at, dppr_ftrack_sample, dppr_debug_ftrack_rank): declared in include/dppr.h with their contract, exported by the
library, listed in engine.EXPORTS with their prototypes, rejected without a handle with nothing written; the HIP-free plan
(dynamicppr_amd/csrc/dppr_ftrack_rank_plan.hpp) driven by tests/native/ftrack_rank_plan_test.cpp as a stand-alone program under the
address and undefined-behaviour sanitizers; ./pagerank --forward-rank accepted and refused; and the numpy glue
(tests/ftrack_rank_ref.py) on a 6-vertex case worked by hand. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import ftrack_rank_ref as frr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_ftrack_topk_ranked", "dppr_ftrack_rank_score_at", "dppr_ftrack_position_at", "dppr_ftrack_sample", "dppr_debug_ftrack_rank")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    flat = " ".join(text.replace("\n *", " ").split())
    for phrase in ("There is no `epoch` argument", "exactly what dppr_ftrack_read returns at v (at_p)", "holds 0.15 * w", "a parked vertex keeps its value",
                   "p may be negative", "0 for a vertex without a live row", "word for word THE SCORE of dppr_topk_ranked", "scores exactly +0.0",
                   "the ids dppr_ftrack_info lists for it, whatever their weights", "Exclusion is per column",
                   "THE ONE PLACE this differs from the NO ID rule", "DPPR_EXCLUDE_SEEDS takes it out although it has no row",
                   "with \"lane\" read as \"column\"", "the lane index i = the column", "m * S <= DPPR_SAMPLE_MAX_TOTAL",
                   "never looks at the graph", "left the ring", "not of m, of the other columns, of the grid or of any debug hook",
                   "a column whose only seed is rowless included", "a radix sort against a selection", "no such track",
                   "n_ids > DPPR_POSITION_MAX", "safe beside dppr_slide_concurrent", "read in place by external id", "ONE read of the row count",
                   "no position comes from an atomic", "the compaction cannot change a result", "Zero kept rows is a valid result",
                   "nothing is compacted there", "after DPPR_ERR_NOMEM the track and the engine are as before", "dppr_debug_query_ms reports the call",
                   "a power of two in [64, 1024]", "Every setting gives the same bits",
                   "OUT OF SCOPE: the subgraph, patch and changes families over a track"):
        assert phrase in flat, phrase
    # the three forward sections point at the new calls; the subgraph family over a track stays out of scope
    assert flat.count("dppr_ftrack_topk_ranked and its siblings") == 2 and "dppr_ftrack_topk_ranked / _rank_score_at / _position_at / _sample" in flat
    assert "the ranked and subgraph families over a" not in flat and "the subgraph family over a track" in flat


def test_library_exports_the_calls_with_their_prototypes():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    L = eng.lib()
    assert L.dppr_abi_version() == 6
    assert len(L.dppr_ftrack_topk_ranked.argtypes) == 8 and len(L.dppr_ftrack_rank_score_at.argtypes) == 6
    assert len(L.dppr_ftrack_position_at.argtypes) == 8 and len(L.dppr_ftrack_sample.argtypes) == 13 and len(L.dppr_debug_ftrack_rank.argtypes) == 2
    fn = L.dppr_ftrack_sample
    assert fn.argtypes[3] is ctypes.c_double and fn.argtypes[4] is ctypes.c_uint64 and fn.argtypes[5] is ctypes.c_uint64 and fn.restype is ctypes.c_int
    for name in ("topk_ranked", "rank_score_at", "position_at", "sample"):
        assert callable(getattr(eng.ForwardTrack, name)), name
    assert callable(eng.Engine.debug_ftrack_rank)


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    ints, dbls = np.full(16, 7, dtype=np.int32), np.full(16, 2.5)
    ids = np.array([0, 1], dtype=np.int32)
    assert L.dppr_ftrack_topk_ranked(None, 0, None, 4, 0.0, ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp), ints.ctypes.data_as(ip)) == -1
    assert L.dppr_ftrack_rank_score_at(None, 0, None, ids.ctypes.data_as(ip), 2, dbls.ctypes.data_as(dp)) == -1
    assert L.dppr_ftrack_position_at(None, 0, None, 0.0, ids.ctypes.data_as(ip), 2, ints.ctypes.data_as(ip), ints.ctypes.data_as(ip)) == -1
    assert L.dppr_ftrack_sample(None, 0, None, 0.0, 1, 0, 4, eng.DEST_HOST, ints.ctypes.data, dbls.ctypes.data, dbls.ctypes.data_as(dp),
                                ints.ctypes.data_as(ip), ints.ctypes.data_as(ip)) == -1
    assert L.dppr_debug_ftrack_rank(None, 64) == -1
    assert np.all(ints == 7) and np.all(dbls == 2.5) and ids.tolist() == [0, 1]


def test_ftrack_rank_plan(tmp_path):
    """dppr_ftrack_rank_plan.hpp: every argument rule at its limit, the tiles, stages and grids for V in {1, 63, 64, 65, 1024, 2^22} at
    every legal tile_rows, what the scan asks of the tiles, the seed table, the sizes at V = 2^31 - 1 and m = 16. (The case worked by
    hand is test_reference_on_a_hand_computed_case below.)"""
    exe = str(tmp_path / "ftrack_rank_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "ftrack_rank_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cli_accepts_and_refuses_forward_rank(tmp_path):
    """--forward-rank K needs --forward-track and K in [1, DPPR_TOPK_MAX]; it lets --rank-factor / --rank-exclude stand without
    --topk. A refusal is `invalid arguments` and the usage, before any device work; what is accepted gets past the check."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    srcs, sets = str(tmp_path / "sources.txt"), str(tmp_path / "track.txt")
    open(srcs, "w").write("1\n2\n3\n4\n")
    open(sets, "w").write("1\n2 3:0.5\n")
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2", "--sources", srcs]
    track = ["--forward-track", sets, "--push-eps", "1e-5"]
    for bad in (["--forward-rank", "10"], track + ["--forward-rank", "0"], track + ["--forward-rank", "-3"], track + ["--forward-rank", "8193"],
                track + ["--forward-rank", "10", "--rank-factor", "nonsense"],
                track + ["--forward-rank", "10", "--rank-exclude", "seeds,up"], track + ["--rank-factor", "deg"]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--forward-rank <K>" in r.stdout, (bad, r.stdout[-400:])
        assert "start..." not in r.stdout and "no CPU fallback" not in r.stdout and "franked " not in r.stdout.split("invalid arguments")[0], bad
    for good in (track + ["--forward-rank", "1"], track + ["--forward-rank", "8192"],
                 track + ["--forward-rank", "10", "--rank-factor", "deg", "--rank-exclude", "seeds,out"]):
        r = run(base + good)
        assert "invalid arguments" not in r.stdout, (good, r.stdout[-400:])


def test_reference_on_a_hand_computed_case():
    """Six vertices, one column with the seeds {5 (weight 2), 0 (weight 1)}. Vertex 5 is named by no stored edge: it has no row and
    holds p = 0.15 * 2. Stored edges 0 -> 1, 0 -> 2, 1 -> 2, 2 -> 3, 3 -> 0; vertex 4 is parked: no edge, a kept value."""
    p = np.array([0.2, 0.1, 0.12, 0.05, 0.01, 0.15 * 2.0])
    row, col = np.array([0, 2, 3, 4, 5, 5, 5]), np.array([1, 2, 2, 3, 0])
    g = frr.Graph(6, row, col)
    seeds = [np.array([5, 0])]
    assert g.outdeg.tolist() == [2, 1, 1, 1, 0, 0]
    raw = frr.scores([p], seeds)[0]
    assert frr.topk(raw, 6)[0].tolist() == [5, 0, 2, 1, 3, 4]                         # the rowless seed is first in the raw order
    no_seeds = frr.scores([p], seeds, exclude=frr.SEEDS)[0]                            # (no graph is needed for the seeds alone)
    assert frr.topk(no_seeds, 6)[0].tolist() == [2, 1, 3, 4] and no_seeds[5] == 0.0 and not np.signbit(no_seeds[5])
    pos, cnt = frr.positions([raw, no_seeds], np.array([5, 4, 5, 0]))
    assert pos.tolist() == [[0, -1], [5, 3], [0, -1], [1, -1]] and cnt.tolist() == [6, 4]   # first raw, in no order without the seeds; a duplicate id
    inv = frr.scores([p], seeds, g, factor=frr.INV_DEG)[0]
    assert inv[5] == p[5] / 1.0 and inv[0] == 0.2 / 3.0 and inv[4] == 0.01
    who = frr.scores([p], seeds, g, factor=frr.DEG, exclude=frr.SEEDS | frr.IN_NEIGHBOURS | frr.OUT_NEIGHBOURS)[0]
    assert who.tolist() == [0.0, 0.0, 0.0, 0.0, 0.01, 0.0]                              # 1, 2: seed -> v; 3: v -> seed; 4: parked, outdeg 0
    allow = np.array([0, 1, 0, 1, 1, 1], dtype=np.uint8)
    masked = frr.scores([p], seeds, g, factor=frr.DEG, allow=allow)[0]
    assert masked.tolist() == [0.0, 0.1 * 2.0, 0.0, 0.05 * 2.0, 0.01, p[5]]
    ids, w, total, support, status = frr.sample([no_seeds], 64, seed=3)
    assert status.tolist() == [0] and support.tolist() == [4] and set(ids[0]) <= {1, 2, 3, 4} and total[0] == (0.1 + (0.12 + 0.05)) + 0.01
    empty = frr.sample([np.where(np.arange(6) == 5, no_seeds, 0.0)], 4)
    assert empty[4].tolist() == [1] and empty[0].tolist() == [[-1, -1, -1, -1]]         # the rowless seed alone, excluded: EMPTY
