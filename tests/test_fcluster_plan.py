"""CPU-side checks of the full-length conductance sweep of a forward track (dppr_ftrack_cluster): declared in include/dppr.h with its
contract, exported by the library, listed in engine.EXPORTS, rejected without a handle; the HIP-free plan
(dynamicppr_amd/csrc/dppr_fcluster_plan.hpp) driven by tests/native/fcluster_plan_test.cpp as a stand-alone program under the address
and undefined-behaviour sanitizers, its host restatement of order -> differences -> scan -> best held against tests/fcluster_ref.py
bit for bit on the 60-vertex stream of tests/test_ftrack_ref.py; and tests/fcluster_ref.py itself against the SET definition
(cluster_ref.brute_arrays). No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import cluster_ref as cr
from tests import fcluster_ref as fcr
from tests import forward_ref as fr
from tests import ftrack_ref as tr
from tests.test_ftrack_ref import BATCHES, LAST, LATE, SETS, V, records, small_stream, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_ftrack_cluster", "dppr_debug_ftrack_cluster")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    assert re.search(r"^#define DPPR_FCLUSTER_BY_P\s+0\b", code, re.M) and re.search(r"^#define DPPR_FCLUSTER_BY_P_OVER_DEG\s+1\b", code, re.M)
    assert re.search(r"\}\s*dppr_fcluster_t;", code)
    for phrase in ("score = p[v] / (double)(outdeg(v) + 1), ONE division", "at least one stored edge of the epoch names it",
                   "a +-0 score and a NaN score never qualify", "+infinity\n *             orders first", "score descending, external id ascending",
                   "a self loop never\n *             crosses a cut", "the first minimum", "the arrays of a smaller max_len are the head",
                   "always written, with the TRUE counts", "the size-and-best query", "ONE read of the per-column counts",
                   "none from the return\n *             value of an atomic", "Every setting gives the same bits", "the track's epoch no longer resident"):
        assert phrase in text, phrase
    # the three forward sections point here now; ranked and subgraph stay out of scope
    assert text.count("dppr_ftrack_cluster.)") == 3 and "ranked, cluster" not in text


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    assert callable(eng.ForwardTrack.cluster) and callable(eng.Engine.debug_ftrack_cluster)
    assert ctypes.sizeof(eng.FCluster) == 40 and eng.FCluster.best_phi.offset == 32
    assert eng.FCLUSTER_ORDERS == {"p": 0, "deg": 1}


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    best = np.full(5 * 2, 7, dtype=np.int64)
    off, ids = np.full(3, 7, dtype=np.int64), np.full(8, 7, dtype=np.int32)
    assert L.dppr_ftrack_cluster(None, 0, 1, 0.0, 0, 1, 8, 0, best.ctypes.data, off.ctypes.data, ids.ctypes.data, None, None, None, None) == -1
    assert L.dppr_debug_ftrack_cluster(None, 64, 64) == -1
    assert np.all(best == 7) and np.all(off == 7) and np.all(ids == 7)


def hexbits(x):
    return "%016x" % np.float64(x).view(np.uint64)


def stream_states():
    """(out-rows, [p of every column]) of the 60-vertex stream: after the create (five rounds: unconverged) and after batches that
    leave p signed, remove LAST's only edge and first name LATE."""
    t, h = small_stream()
    eps = (1e-6, 1e-3, 1e-8)
    rows = fr.Rows.from_edges(V, *window(t, h, 0))
    cols = [tr.Column(rows, ids, w, e, 5) for (ids, w), e in zip(SETS, eps)]
    out = [(fcr.out_rows(V, *window(t, h, 0)), [c.p.copy() for c in cols])]
    for k in range(1, BATCHES + 1):
        rows = fr.Rows.from_edges(V, *window(t, h, k))
        for c in cols:
            c.update(rows, records(t, h, k), 64)
        if k in (1, 3, 5, 12, BATCHES):
            out.append((fcr.out_rows(V, *window(t, h, k)), [c.p.copy() for c in cols]))
    return out


def test_the_reference_against_the_set_definition():
    states = stream_states()
    assert any(np.any(p < 0) for _, ps in states for p in ps)                      # p is signed after deletes
    (ptr0, col0), ps0 = states[0]
    assert ps0[1][LATE] == 0.15 * 0.5 and ptr0[LATE + 1] == ptr0[LATE] and LATE not in col0   # a rowless seed holds p and is in no order
    for (ptr, col), ps in states:
        for p in ps:
            for order in ("p", "deg"):
                best, ids, s, co, ci, vol = fcr.cluster(p, ptr, col, order)
                assert LATE not in ids or (ptr[LATE + 1] > ptr[LATE] or LATE in col)
                assert np.all(s > 0) and np.all(np.diff(s) <= 0) and np.all((np.diff(s) < 0) | (np.diff(ids) > 0))
                bo, bi, bv = cr.brute_arrays(V, ptr, col, ids)
                assert np.array_equal(co, bo) and np.array_equal(ci, bi) and np.array_equal(vol, bv)
                assert best["count"] == len(ids) and (best["best_size"] == 0 or best["best_cut"] == co[best["best_size"] - 1])
    (ptr, col), ps = states[2]
    assert LAST not in fcr.ordered(ps[1], ptr, col, "p")[0] and ps[1][LAST] != 0.0    # LAST lost its only edge: p stays, the order drops it


def test_fcluster_plan_and_the_host_restatement_against_numpy(tmp_path):
    exe = str(tmp_path / "fcluster_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "fcluster_plan_test.cpp")])
    states = stream_states()
    n_lines = 0
    for si, ((ptr, col), ps) in enumerate(states):
        cases, text = [], ["%d %d" % (V, ptr[-1]), " ".join(map(str, ptr)), " ".join(map(str, col))]
        for p in ps:
            for order in (0, 1):
                for min_score, max_len, min_size, tile in ((0.0, 0, 1, 64), (0.0, 0, 1, 4), (0.0, 0, 1, 1), (1e-4, 0, 3, 16), (0.0, 7, 1, 4),
                                                           (0.0, 37, 2, 8)):
                    cases.append((p, order, min_score, max_len, min_size))
                    text.append("%d %s %d %d %d" % (order, hexbits(min_score), max_len, min_size, tile))
                    text.append(" ".join(hexbits(x) for x in p))
        text.insert(3, str(len(cases)))
        case = tmp_path / ("case%d.txt" % si)
        case.write_text("\n".join(text) + "\n")
        r = subprocess.run([exe, str(case)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith("res ")]
        assert len(lines) == len(cases)
        for l, (p, order, min_score, max_len, min_size) in zip(lines, cases):
            want = fcr.cluster(p, ptr, col, order, min_score, max_len, min_size)
            best = dict(count=int(l[2]), best_size=int(l[3]), best_cut=int(l[4]), best_vol=int(l[5]),
                        best_phi=float(np.uint64(int(l[6], 16)).view(np.float64)))
            rest = l[7:]
            got = (best, np.array(rest[0::5], dtype=np.int32), np.array([int(x, 16) for x in rest[1::5]], dtype=np.uint64).view(np.float64),
                   np.array(rest[2::5], dtype=np.int64), np.array(rest[3::5], dtype=np.int64), np.array(rest[4::5], dtype=np.int64))
            fcr.same(got, want, (si, l[1]))
            n_lines += 1
    assert n_lines == len(states) * len(SETS) * 2 * 6
