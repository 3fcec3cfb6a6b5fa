"""CPU-side checks of the lane-axis query (dppr_assign, dppr_assign_at): declared in include/dppr.h with their contract, exported
by the library, listed in engine.EXPORTS with their prototypes, rejected without a handle with nothing written; the HIP-free plan
(dynamicppr_amd/csrc/dppr_assign_plan.hpp) driven by tests/native/assign_plan_test.cpp as a stand-alone program under the address
and undefined-behaviour sanitizers; the refusals of ./pagerank --assign; and the numpy reference (tests/assign_ref.py) on a case
worked out by hand. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import assign_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_assign", "dppr_assign_at")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    assert re.search(r"^#define DPPR_ASSIGN_GROUPS_MAX\s+16\b", code, re.M) and re.search(r"^#define DPPR_ASSIGN_CLASSES_MAX\s+256\b", code, re.M)
    assert (eng.ASSIGN_GROUPS_MAX, eng.ASSIGN_CLASSES_MAX) == (16, 256)
    # the contract is stated where a caller reads it
    for phrase in ("ONE multiplication", "ONE subtraction", "the SMALLEST class", "starts at +0.0", "a strictly greater score", "never win",
                   "always the TRUE", "NOTHING is", "counts only", "may BE out_label", "No output position comes from an atomic",
                   "m == 0 is a valid no-op", "obtained before anything is written", "OUT OF SCOPE", "A group may be named twice",
                   "needs no resident epoch"):
        assert phrase in text, phrase


def test_library_exports_the_calls_with_their_prototypes():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    L = eng.lib()
    assert L.dppr_abi_version() == 6
    assert len(L.dppr_assign.argtypes) == 16 and len(L.dppr_assign_at.argtypes) == 11
    assert L.dppr_assign.restype is ctypes.c_int and L.dppr_assign_at.restype is ctypes.c_int
    assert L.dppr_assign.argtypes[4] is ctypes.c_double and L.dppr_assign.argtypes[11] is ctypes.c_int64
    for name in ("assign", "assign_dev", "assign_at"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip, dp, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    groups = np.zeros(1, dtype=np.int32)
    label, best, margin = np.full(4, 7, dtype=np.int32), np.full(4, 2.5), np.full(4, 3.5)
    counts, nf = np.full(3, 7, dtype=np.int64), np.full(1, 7, dtype=np.int64)
    lists = [np.full(4, 7, dtype=np.int32) for _ in range(3)]
    at = np.array([0, 1], dtype=np.int32)
    assert L.dppr_assign(None, groups.ctypes.data_as(ip), 1, None, 0.0, 0, label.ctypes.data, best.ctypes.data, margin.ctypes.data,
                         counts.ctypes.data_as(i64p), label.ctypes.data, 4, nf.ctypes.data_as(i64p), *(a.ctypes.data for a in lists)) == -1
    assert L.dppr_assign_at(None, groups.ctypes.data_as(ip), 1, None, 0.0, at.ctypes.data_as(ip), 2, label.ctypes.data_as(ip),
                            best.ctypes.data_as(dp), lists[0].ctypes.data_as(ip), margin.ctypes.data_as(dp)) == -1
    assert np.all(label == 7) and np.all(best == 2.5) and np.all(margin == 3.5) and np.all(counts == 7) and np.all(nf == 7)
    assert all(np.all(a == 7) for a in lists)


def test_assign_plan(tmp_path):
    """dppr_assign_plan.hpp: block layouts that do not overlap and are aligned for C in {1, 16, 17, 256}, tile counts at V in
    {1, 255, 256, 257}, the class table, the team of a row width, every argument rule at its limit."""
    exe = str(tmp_path / "assign_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "assign_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cli_refuses_assign_without_groups_on_one_device(tmp_path):
    """--assign with the lanes dealt over two engines (-g 2), with one source (no group), with --no-groups / --split, a negative
    --assign-min, or --assign-min / --assign-out without --assign: invalid arguments and the usage, before any device work."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    srcs = str(tmp_path / "sources.txt")
    open(srcs, "w").write("1\n2\n3\n4\n")
    sets = str(tmp_path / "sets.txt")
    open(sets, "w").write("1 2:0.5\n3\n")
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2"]
    for bad in (["--assign", "--sources", srcs, "-g", "2"], ["--assign", "--target-sets", sets, "-g", "2"], ["--assign", "-s", "1"], ["--assign"],
                ["--assign", "--sources", srcs, "--no-groups"], ["--assign", "--sources", srcs, "--split"],
                ["--assign", "--sources", srcs, "--assign-min", "-0.5"], ["--sources", srcs, "--assign-min", "0.1"],
                ["--sources", srcs, "--assign-out", str(tmp_path / "labels.bin")]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--assign [--assign-min <S>] [--assign-out <file>]" in r.stdout, (bad, r.stdout[-400:])
        assert "start..." not in r.stdout and "no CPU fallback" not in r.stdout, (bad, r.stdout[-400:])


def test_reference_on_a_hand_computed_case():
    """Five vertices, four classes. Every number below was worked out by hand from the definition of include/dppr.h."""
    p = np.array([[0.5, 0.25, 0.5, 0.125],      # a tie of classes 0 and 2: the smallest wins, the other is second, the margin is +0.0
                  [0.0, 0.0, 0.0, 0.0],         # nothing: unassigned
                  [0.125, -0.5, 0.0, 0.25],     # a negative score never counts
                  [0.0, 0.75, 0.0, 0.0],        # one positive score: second stays +0.0
                  [0.0625, 0.0625, 0.03125, 0.0]])
    label, best, second, second_label, margin = ref.assign(p)
    assert label.tolist() == [0, -1, 3, 1, 0] and label.dtype == np.int32
    assert best.tolist() == [0.5, 0.0, 0.25, 0.75, 0.0625]
    assert second.tolist() == [0.5, 0.0, 0.125, 0.0, 0.0625] and second_label.tolist() == [2, -1, 0, -1, 1]
    assert margin.tolist() == [0.0, 0.0, 0.125, 0.75, 0.0] and not np.signbit(margin).any()
    assert ref.counts(label, 4).tolist() == [2, 1, 0, 1, 1]
    # a threshold: the label needs a score above it, the runner-up does not; without a label best = margin = +0.0
    label, best, second, second_label, margin = ref.assign(p, min_score=0.25)
    assert label.tolist() == [0, -1, -1, 1, -1] and best.tolist() == [0.5, 0.0, 0.0, 0.75, 0.0] and margin.tolist() == [0.0, 0.0, 0.0, 0.75, 0.0]
    assert second_label.tolist() == [2, -1, 3, -1, 0] and second.tolist() == [0.5, 0.0, 0.25, 0.0, 0.0625]
    # scales: one multiplication per score; a class scaled by zero never wins
    scale = np.array([0.0, 2.0, 1.0, 4.0])
    label, best, second, second_label, margin = ref.assign(p, scale)
    assert label.tolist() == [1, -1, 3, 1, 1] and best.tolist() == [0.5, 0.0, 1.0, 1.5, 0.125]
    assert second_label.tolist() == [2, -1, -1, -1, 2] and margin.tolist() == [0.0, 0.0, 1.0, 1.5, 0.09375]
    assert np.array_equal(ref.bits(ref.scores(p, np.ones(4))), ref.bits(ref.scores(p)))
    # flips: ascending ids, old and new
    ids, old, new = ref.flips(np.array([0, -1, 2, 1, 1]), np.array([0, -1, 3, 1, 0]))
    assert ids.tolist() == [2, 4] and old.tolist() == [2, 1] and new.tolist() == [3, 0] and ids.dtype == np.int32
