"""CPU-side checks of the forward track (dppr_ftrack_create / _update / _read / _info / _destroy): declared in include/dppr.h with their
contract, exported by the library, listed in engine.EXPORTS, rejected without a handle; the HIP-free plan
(dynamicppr_amd/csrc/dppr_ftrack_plan.hpp) driven by tests/native/ftrack_plan_test.cpp as a stand-alone program under the address and
undefined-behaviour sanitizers, its host restatement of create, fix-up and signed rounds held against tests/ftrack_ref.py bit for bit
on the 60-vertex stream of tests/test_ftrack_ref.py. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import forward_ref as fr
from tests import ftrack_ref as tr
from tests.test_ftrack_ref import BATCHES, SETS, V, records, small_stream, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_ftrack_create", "dppr_ftrack_update", "dppr_ftrack_read", "dppr_ftrack_info", "dppr_ftrack_destroy")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    assert re.search(r"^#define DPPR_FTRACK_MAX\s+16\b", code, re.M) and eng.FTRACK_MAX == 16
    assert re.search(r"\}\s*dppr_ftrack_out_t;", code) and re.search(r"\bfix\s*;", code)
    for phrase in ("F = { u : |r[u]| > thr[u] }, strict", "g[u] = p[u] / (0.15 * (double)(d0 + 1))", "c[u] = 0.85 * g[u]",
                   "p[u] = (p[u] * (double)(d1 + 1)) / (double)(d0 + 1)", "r[u] = r[u] - (double)(d1 - d0) * g[u]",
                   "A tail with d1 == d0 keeps p[u] and r[u] to the bit", "sequential, one rounding per record", "r is never -0.0",
                   "THE FOLD of |r| over the external ids", "a fresh track equals dppr_forward_push", "accepts exactly two epochs",
                   "with the track unchanged", "planes by EXTERNAL id", "never blocks a renumbering",
                   "No output\n * value comes from a floating-point atomic"):
        assert phrase in text, phrase
    assert "keeping a forward vector current under the stream" not in text   # the two OUT OF SCOPE lines name the track now


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    assert callable(eng.Engine.ftrack)
    for name in ("update", "read", "info", "close"):
        assert callable(getattr(eng.ForwardTrack, name)), name
    o, q = eng.FtrackOut, eng.ForwardPushOut
    assert ctypes.sizeof(o) == 152 and o.fix.offset == ctypes.sizeof(q) == 144
    for f, _ in q._fields_:
        assert getattr(o, f).offset == getattr(q, f).offset, f


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip, dp, lp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    guard, iguard = np.full(8, 7.0), np.full(8, 7, dtype=np.int32)
    off, ids, w = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.ones(2)
    out = eng.FtrackOut()
    out.rounds_used, out.rem = iguard.ctypes.data_as(ip), guard.ctypes.data_as(dp)
    t = ctypes.c_int32(7)
    assert L.dppr_ftrack_create(None, -1, off.ctypes.data_as(lp), ids.ctypes.data_as(ip), w.ctypes.data_as(dp), 2, 1e-6, 8, ctypes.byref(out),
                                ctypes.byref(t)) == -1
    assert L.dppr_ftrack_update(None, 0, -1, 8, ctypes.byref(out)) == -1 and L.dppr_ftrack_read(None, 0, ctypes.byref(out)) == -1
    assert L.dppr_ftrack_destroy(None, 0) == -1 and L.dppr_ftrack_info(None, 0, None, None, None, None, None, None, 0) == -1
    assert np.all(guard == 7.0) and np.all(iguard == 7) and t.value == 7


def hexbits(x):
    return "%016x" % np.float64(x).view(np.uint64)


def graph_text(rows):
    return "\n".join([str(len(rows.tails)), " ".join(map(str, rows.ptr)), " ".join(map(str, rows.tails)), " ".join(str(int(d)) for d in rows.d)])


# (kind, max_rounds) of the steps after the create: a batch each, a few of them cut short and finished on the own epoch
def steps():
    out = []
    for k in range(1, BATCHES + 1):
        cap = 2 if k in (3, 9) else 64
        out.append((1, cap, k))
        if cap == 2:
            out += [(0, 1, k), (0, 64, k)]
    return out


def test_ftrack_plan_and_the_host_restatement_against_numpy(tmp_path):
    exe = str(tmp_path / "ftrack_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "ftrack_plan_test.cpp")])
    t, h = small_stream()
    eps, rounds0 = (1e-6, 1e-3, 1e-8), 5     # (five rounds leave the create unconverged: the first fix-up meets such a track)
    rows = fr.Rows.from_edges(V, *window(t, h, 0))
    st = steps()
    text = ["%d %d %d %d" % (V, len(SETS), len(st), rounds0)]
    for (ids, w), e in zip(SETS, eps):
        text.append(hexbits(e) + " %d " % len(ids) + " ".join("%d %s" % (int(q), hexbits(x)) for q, x in zip(ids, w)))
    text.append(graph_text(rows))
    cols = [tr.Column(rows, ids, w, e, rounds0) for (ids, w), e in zip(SETS, eps)]
    want = [[(c.p.copy(), c.r.copy(), c.last) for c in cols]]
    assert any(c.last.converged == 0 for c in cols)
    for kind, cap, k in st:
        text.append("%d %d" % (kind, cap))
        rec = None
        if kind == 1:
            rec = records(t, h, k)
            rows = fr.Rows.from_edges(V, *window(t, h, k))
            text.append(str(len(rec[0])) + "\n" + "\n".join("%d %d %d" % x for x in zip(*rec)) + "\n" + graph_text(rows))
        for c in cols:
            c.update(rows, rec, cap)
        want.append([(c.p.copy(), c.r.copy(), c.last) for c in cols])
    case = tmp_path / "case.txt"
    case.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(case)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("state ")]
    assert len(lines) == (len(st) + 1) * len(SETS)
    for l in lines:
        s, ci = int(l[1]), int(l[2])
        p, rr, last = want[s][ci]
        assert [int(x) for x in l[3:9]] == [last.rounds_used, last.pushes, last.left] + last.fix, (s, ci, l[3:9])
        gp = np.array([int(x, 16) for x in l[9::2]], dtype=np.uint64)
        gr = np.array([int(x, 16) for x in l[10::2]], dtype=np.uint64)
        assert np.array_equal(gp, p.view(np.uint64)) and np.array_equal(gr, rr.view(np.uint64)), (s, ci)
    assert any(w[2].converged == 0 for ws in want[1:] for w in ws) and all(w[2].converged == 1 for w in want[-1])
