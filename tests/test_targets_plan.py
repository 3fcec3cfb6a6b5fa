"""CPU-side checks of weighted vertex sets as the targets of a group (dppr_add_target_group, dppr_group_replace_target,
dppr_group_targets): declared in include/dppr.h with DPPR_TARGET_SET_MAX, exported by the library, listed in engine.EXPORTS,
rejected without a handle; the HIP-free plan (dynamicppr_amd/csrc/dppr_targets_plan.hpp) driven by
tests/native/targets_plan_test.cpp as a stand-alone program under the address and undefined-behaviour sanitizers; and the numpy
reference (tests/targets_ref.py) pinned to the oracle: its fixed point for a one-hot h is the oracle's power iteration, and the
oracle's own frontier loop started from p = 0, r = h ends within eps of it. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import targets_ref
from tests.util import window_directed_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_add_target_group", "dppr_group_replace_target", "dppr_group_targets")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    assert re.search(r"^#define DPPR_TARGET_SET_MAX 65536\b", code, re.M) and eng.TARGET_SET_MAX == 65536
    # the contract is stated where a caller reads it
    for phrase in ("LINEAR IN THE TARGET", "|p - exact| < eps FOR ANY h", "finite and > 0", "is a source lane", "reports -1",
                   "ALWAYS written", "never parked", "the same id in different lanes is fine", "as it was before the call"):
        assert phrase in text, phrase


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("add_target_group", "group_replace_target", "group_targets"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    off = np.array([0, 1], dtype=np.int64)
    ids, w = np.array([3], dtype=np.int32), np.array([1.0])
    gid = ctypes.c_int32(7)
    i64p, ip, dp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    assert L.dppr_add_target_group(None, off.ctypes.data_as(i64p), ids.ctypes.data_as(ip), w.ctypes.data_as(dp), 1, ctypes.byref(gid)) == -1
    assert L.dppr_group_replace_target(None, 0, 0, ids.ctypes.data_as(ip), w.ctypes.data_as(dp), 1, None) == -1
    out = np.full(17, 7, dtype=np.int64)
    assert L.dppr_group_targets(None, 0, out.ctypes.data_as(i64p), None, None, 0) == -1
    assert gid.value == 7 and np.all(out == 7)


def test_seed_sets_of_the_binding():
    ids, w = eng.Engine._seed_set(5)
    assert ids.tolist() == [5] and w.tolist() == [1.0] and ids.dtype == np.int32
    ids, w = eng.Engine._seed_set([4, 2])
    assert ids.tolist() == [4, 2] and w.tolist() == [1.0, 1.0]
    ids, w = eng.Engine._seed_set(([4, 2], [0.25, 0.75]))
    assert ids.tolist() == [4, 2] and w.tolist() == [0.25, 0.75] and w.dtype == np.float64
    with pytest.raises(ValueError):
        eng.Engine._seed_set(([4, 2], [0.25]))


def test_targets_plan(tmp_path):
    """dppr_targets_plan.hpp: every rejection at its limit, the mirror, the table, the lookup, remap == rebuild, the lane changes."""
    exe = str(tmp_path / "targets_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "targets_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


@pytest.fixture(scope="module")
def window():
    V, e1, e2 = datagen.rmat_stream(10, 12000, 3)
    return V, e1, e2, 4000, 100


@pytest.mark.parametrize("directed", [1, 0])
def test_exact_p_of_a_one_hot_h_is_the_power_iteration(window, directed):
    """(measured on R-MAT scale 12, W = 30 000: 5e-14)"""
    V, e1, e2, W, c = window
    g = orc.Graph(V, e1, e2, directed, W, c)
    src, dst = window_directed_edges(g)
    for s in (int(e1[0]), int(e2[5]), V - 1):
        h = targets_ref.seed_vector([s], [1.0], V)
        want, _ = orc.pow_rev(g, s)
        gap = float(np.max(np.abs(targets_ref.exact_p(h, src, dst, V) - want)))
        print("one-hot gap", directed, s, gap)
        assert gap < 1e-12
        assert targets_ref.invariant_err(want, np.zeros(V), h, src, dst, V) < 1e-12


@pytest.mark.parametrize("directed", [1, 0])
@pytest.mark.parametrize("m", [2, 40, 300])
def test_oracle_loop_from_the_seeded_init_ends_within_eps_of_exact_p(window, directed, m):
    """Init for a set lane (p = 0, r = h) and the oracle's own phase-0 loop: max|r| < eps, no negative residual, the invariant with
    h, and |p - exact_p| < eps (the bound derived in include/dppr.h)."""
    V, e1, e2, W, c = window
    eps = 1e-9
    g = orc.Graph(V, e1, e2, directed, W, c)
    src, dst = window_directed_edges(g)
    rng = np.random.default_rng(100 + m)
    ids = rng.choice(V, m, replace=False)
    w = rng.random(m) + 0.01
    h = targets_ref.seed_vector(ids, w / w.sum(), V)
    s = orc.State(V, 0, eps)
    s.p[:] = 0.0
    s.r[:] = h
    s.sync_main_loop(g, 0)
    p, r = s.p.copy(), s.r.copy()
    assert np.max(np.abs(r)) < eps and r.min() >= 0.0
    assert targets_ref.invariant_err(p, r, h, src, dst, V) < 1e-13
    gap = float(np.max(np.abs(p - targets_ref.exact_p(h, src, dst, V))))
    print("seeded init gap", directed, m, gap)
    assert gap < eps


def test_cli_target_sets_arguments(tmp_path):
    """--target-sets beside --sources, --split, --no-groups or --topk-weights, a file that is missing, a blank line and a token that
    is no id[:weight]: invalid arguments and the usage, before any device work."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    good, src = tmp_path / "sets.txt", tmp_path / "src.txt"
    good.write_text("1 2:0.5\n3\n")
    src.write_text("1\n2\n")
    blank, token = tmp_path / "blank.txt", tmp_path / "token.txt"
    blank.write_text("1 2\n\n3\n")
    token.write_text("1 2:x\n")
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2"]
    for bad in (["--target-sets", str(good), "--sources", str(src)], ["--target-sets", str(good), "--split"],
                ["--target-sets", str(good), "--no-groups"], ["--target-sets", str(good), "--topk", "3", "--topk-weights", "1,1"],
                ["--target-sets", str(tmp_path / "missing.txt")], ["--target-sets", str(blank)], ["--target-sets", str(token)]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--target-sets <file>" in r.stdout, (bad, r.stdout[-400:])
