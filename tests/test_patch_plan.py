"""CPU-side checks of the patch feed (dppr_patch / dppr_group_patch): declared in include/dppr.h with its modes and its out
block, exported by the library, listed in engine.EXPORTS with prototypes, rejected without a handle with nothing written; the
command line's rejections; the HIP-free plan of a call (dynamicppr_amd/csrc/dppr_patch_plan.hpp) driven by
tests/native/patch_plan_test.cpp as a stand-alone program under the address and undefined-behaviour sanitizers; and the numpy
restatement itself (tests/patch_ref.py), worked by hand and held to the property that the emitted-only re-mark bounds drift. No
GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import patch_ref as ref
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_patch", "dppr_group_patch")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, value in (("DPPR_PATCH_KEEP_MARK", 0), ("DPPR_PATCH_REMARK_ALL", 1), ("DPPR_PATCH_REMARK_EMITTED", 2)):
        assert re.search(rf"^#define {name} {value}\b", code, re.M), name
    assert (eng.PATCH_KEEP_MARK, eng.PATCH_REMARK_ALL, eng.PATCH_REMARK_EMITTED) == (0, 1, 2)
    struct = re.search(r"typedef struct \{([^}]*)\}\s*dppr_patch_out_t;", code)
    assert struct
    fields = re.findall(r"(\w+)\s*;", struct.group(1))
    assert fields == [f for f, _ in eng.PatchOut._fields_] == ["up_offsets", "up_ids", "up_p", "del_offsets", "del_ids", "written"]
    assert "DPPR_PATCH_REMARK_EMITTED is the mode that BOUNDS DRIFT" in text  # the header says which mode a feed uses, and why


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    L = eng.lib()
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int64,
                               ctypes.c_int, ctypes.c_int, ctypes.c_void_p], name
    assert L.dppr_abi_version() == 6
    for name in ("patch", "group_patch", "patch_dev", "group_patch_dev"):
        assert callable(getattr(eng.Engine, name)), name
    assert callable(eng.apply_patch)


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    uo = (ctypes.c_int64 * 3)(-7, -7, -7)
    do = (ctypes.c_int64 * 3)(-9, -9, -9)
    ids = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    dl = (ctypes.c_int32 * 4)(8, 8, 8, 8)
    p = (ctypes.c_double * 4)(2.5, 2.5, 2.5, 2.5)
    A = ctypes.addressof
    out = eng.PatchOut(uo, A(ids), A(p), do, A(dl), 55)
    for fn in (L.dppr_patch, L.dppr_group_patch):
        for remark in (0, 1, 2):
            assert fn(None, 0, 0.0, 0.0, 4, 4, eng.DEST_HOST, remark, ctypes.byref(out)) == -1
    assert list(uo) == [-7] * 3 and list(do) == [-9] * 3 and list(ids) == [7] * 4 and list(dl) == [8] * 4 and list(p) == [2.5] * 4
    assert out.written == 55


def test_cli_rejects_bad_patch_flags(pagerank, small_bin):
    base = ["-d", small_bin[0], "-a", "0", "-i", "0", "-y", "1", "-n", "0", "-r", "0.01", "-b", "3"]
    for bad in (["--patch-min", "-1"], ["--patch-min", "abc"], ["--patch-min", "1e-6x"], ["--patch-min", "nan"],
                ["--patch-min", "1e-6", "--patch-delta", "-1e-9"], ["--patch-min", "1e-6", "--patch-delta", "x"],
                ["--patch-delta", "1e-9"], ["--patch-out", "x.txt"], ["--patch-min", "1e-6", "--changes", "5"]):
        r = run([pagerank] + base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "[USAGE]" in r.stdout, bad
        assert "--patch-min <P>" in r.stdout
        assert "sliding window size" not in r.stdout, bad  # before the workload is derived, so before any device work
    assert not os.path.exists("x.txt")


def test_patch_plan(tmp_path):
    """dppr_patch_plan.hpp: the workspace, the block at caps of 0, 1 and odd counts (no overlap, 8-byte sections at multiples of 8),
    64-bit sizes, and every rejection at its limit."""
    exe = str(tmp_path / "patch_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "patch_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_the_reference_worked_by_hand():
    """6 ids, 2 lanes, tau = 0.25, delta = 0.125 (both exact in binary)."""
    tau, delta = 0.25, 0.125
    up_tau, dn_tau = np.nextafter(tau, 1.0), np.nextafter(tau, 0.0)
    nan = float("nan")
    #            id 0: new      1: changed > delta   2: changed < delta   3: left    4: |d| == delta      5: untouched below
    m0 = np.array([0.0,         0.5,                 0.5,                 0.5,       0.5,                 0.125])
    p0 = np.array([0.5,         0.75,                0.5625,              0.125,     0.625,               0.125])
    #            id 0: p == tau over a mark above: delete       1: p just above tau over mark == tau: a new entry
    #               2: p just below tau over a mark just above: delete         3: NaN p over a qualifying mark: delete
    #               4: qualifying p over a NaN mark: upsert                    5: -0.0 over 0.0: nothing
    m1 = np.array([up_tau,      tau,                 up_tau,              0.5,       nan,                 0.0])
    p1 = np.array([tau,         up_tau,              dn_tau,              nan,       0.5,                 -0.0])
    pt = ref.patch([p0, p1], [m0, m1], tau, delta)
    assert pt["up_offsets"].tolist() == [0, 2, 4] and pt["del_offsets"].tolist() == [0, 1, 4]
    assert pt["up_ids"].tolist() == [0, 1, 1, 4] and pt["del_ids"].tolist() == [3, 0, 2, 3]
    assert np.array_equal(ref.bits(pt["up_p"]), ref.bits([0.5, 0.75, up_tau, 0.5]))
    assert pt["up_ids"].dtype == np.int32 and pt["del_ids"].dtype == np.int32 and pt["up_offsets"].dtype == np.int64
    assert ref.kinds([p0, p1], [m0, m1], tau, delta) == {"new": 3, "changed": 1, "deleted": 4, "suppressed": 2}
    # delta = 0: the two suppressed entries are sent
    assert ref.patch([p0], [m0], tau, 0.0)["up_ids"].tolist() == [0, 1, 2, 4]
    # the replica: the export of the mark, patched, is the export of the state except at the suppressed entries, which keep the old value
    with_nan_mark = ref.export([m0, m1], tau)
    assert with_nan_mark[1].tolist() == [1, 2, 3, 4, 0, 2, 3]  # (a NaN mark is not in the replica)
    got = ref.apply(with_nan_mark, pt)
    want = ref.export([p0, p1], tau)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].tolist() == [0, 1, 2, 4, 1, 4]
    assert got[2].tolist() == [0.5, 0.75, 0.5, 0.5, up_tau, 0.5] and want[2].tolist() == [0.5, 0.75, 0.5625, 0.625, up_tau, 0.5]
    assert ref.same_sparse(eng.apply_patch(with_nan_mark, pt), got)  # the binding's merge is the same function
    # the three re-marks
    keep, every, emitted = (ref.remark([p0, p1], [m0, m1], tau, delta, mode) for mode in (0, 1, 2))
    assert np.array_equal(ref.bits(keep[0]), ref.bits(m0)) and np.array_equal(ref.bits(keep[1]), ref.bits(m1))
    assert np.array_equal(ref.bits(every[0]), ref.bits(p0)) and np.array_equal(ref.bits(every[1]), ref.bits(p1))
    assert np.array_equal(ref.bits(emitted[0]), ref.bits([0.5, 0.75, 0.5, 0.125, 0.5, 0.125]))
    assert np.array_equal(ref.bits(emitted[1]), ref.bits([tau, up_tau, dn_tau, nan, 0.5, 0.0]))
    # after a re-mark of either kind, delta = 0 or not, the patch of the same state against the new mark is empty
    for mark in (every, emitted):
        again = ref.patch([p0, p1], mark, tau, delta)
        assert again["up_offsets"][-1] == 0 and again["del_offsets"][-1] == 0


def test_the_emitted_only_remark_bounds_drift_and_the_full_remark_does_not():
    """A dense vector walks for 50 steps, every step smaller than delta. Fed with the emitted-only re-mark the replica keeps the exact
    support and stays within delta of p after every step; fed with the full re-mark the same sequence leaves delta behind."""
    rng = np.random.default_rng(7)
    V, tau, delta, steps = 400, 0.3, 0.01, 50
    p = rng.random(V)
    drift = np.where(np.arange(V) % 2 == 0, 0.6, -0.6) * delta  # steady walks: up on the even ids, down on the odd ones
    worst = {}
    for mode in (ref.REMARK_EMITTED, ref.REMARK_ALL):
        now, mark = p.copy(), [p.copy()]
        replica = ref.export([now], tau)
        worst[mode] = 0.0
        sent = 0
        for _ in range(steps):
            step = drift + (rng.random(V) - 0.5) * 0.5 * delta
            assert np.max(np.abs(step)) < delta
            now = now + step
            pt = ref.patch([now], mark, tau, delta)
            sent += len(pt["up_ids"])
            replica = ref.apply(replica, pt)
            mark = ref.remark([now], mark, tau, delta, mode)
            want = ref.export([now], tau)
            assert np.array_equal(replica[0], want[0]) and np.array_equal(replica[1], want[1])  # the support is exact under either mode
            err = float(np.max(np.abs(replica[2] - want[2])))
            worst[mode] = max(worst[mode], err)
            if mode == ref.REMARK_EMITTED:
                assert err <= delta
                held = np.zeros(V, dtype=bool)
                held[replica[1]] = True
                assert np.array_equal(ref.bits(mark[0][held]), ref.bits(replica[2]))  # the mark is what the replica holds
        if mode == ref.REMARK_EMITTED:
            assert 0 < sent < steps * V // 2  # entries were suppressed, and entries were sent again
    assert worst[ref.REMARK_EMITTED] <= delta < worst[ref.REMARK_ALL], worst
    assert worst[ref.REMARK_ALL] > 10 * delta, worst  # 50 steps of 0.6 delta, never seen
