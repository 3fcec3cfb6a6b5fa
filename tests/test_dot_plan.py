"""CPU-side checks of the dot products over the vertex axis (dppr_dot_dense_dev, dppr_dot_sparse and their group forms): declared
in include/dppr.h, exported by the library, listed in engine.EXPORTS, rejected without a handle with nothing written; the HIP-free
plan of a call (dynamicppr_amd/csrc/dppr_dot_plan.hpp) driven by tests/native/dot_plan_test.cpp as a stand-alone program under the
address and undefined-behaviour sanitizers; and the numpy restatement of the fold (tests/dot_ref.py). No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import dot_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_dot_dense_dev", "dppr_group_dot_dense_dev", "dppr_dot_sparse", "dppr_group_dot_sparse")


def test_header_declares_the_four_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, value in (("DPPR_DOT_MAX_F", 4096), ("DPPR_H_FEATURE_MAJOR", 0), ("DPPR_H_VERTEX_MAJOR", 1)):
        assert re.search(rf"^#define {name} {value}\b", code, re.M), name
    assert (eng.DOT_MAX_F, eng.H_FEATURE_MAJOR, eng.H_VERTEX_MAJOR) == (4096, 0, 1)


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("dot_dense_dev", "group_dot_dense_dev", "dot_sparse", "group_dot_sparse", "dot_sparse_dev", "group_dot_sparse_dev"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    off = (ctypes.c_int64 * 3)(0, 1, 2)
    ids = (ctypes.c_int32 * 2)(0, 1)
    w = (ctypes.c_double * 2)(1.0, 1.0)
    out = (ctypes.c_double * 4)(2.5, 2.5, 2.5, 2.5)
    A = ctypes.addressof
    for fn in (L.dppr_dot_dense_dev, L.dppr_group_dot_dense_dev):
        assert fn(None, 0, eng.DENSE_P, A(w), eng.F64, eng.H_FEATURE_MAJOR, 1, eng.DEST_HOST, A(out)) == -1
    for fn in (L.dppr_dot_sparse, L.dppr_group_dot_sparse):
        assert fn(None, 0, eng.DENSE_P, off, A(ids), A(w), eng.DEST_HOST, 2, eng.DEST_HOST, A(out)) == -1
    assert list(out) == [2.5] * 4 and list(off) == [0, 1, 2] and list(ids) == [0, 1] and list(w) == [1.0, 1.0]


def test_dot_plan(tmp_path):
    """dppr_dot_plan.hpp: tile, block and column counts for slot counts {0, 1, 255, 256, 257, 65535, 65536, 65537, 2^22} and mixed
    query lengths, 64-bit sizes beyond 2^31, the argument and offset checks, dot_fold_ref against a plain recursive tree, against the
    crafted cancellation vector and against the fold cut into the device's pieces."""
    exe = str(tmp_path / "dot_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "dot_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_the_numpy_fold_pins_the_order():
    """The helper the GPU tests compare against: the tree, not a running sum and not numpy's dot."""
    t = np.array([1e16, 1.0, -1e16, 1.0])
    assert dot_ref.fold(t) == 0.0 and dot_ref.running(t) == 1.0
    long = np.zeros(600)
    long[8:12] = t
    assert dot_ref.fold(long) == 0.0 and dot_ref.running(long) == 1.0 and float(np.dot(long, np.ones(600))) == 2.0
    for at in (254, 2046, 65534):  # the same four values across a subtile, a tile and a block boundary
        u = np.zeros(at + 4)
        u[at:at + 4] = t
        assert dot_ref.fold(u) == 0.0 and dot_ref.running(u) == 1.0, at
    assert dot_ref.fold(np.zeros((3, 0))).shape == (3,) and np.all(dot_ref.fold(np.zeros((3, 0))) == 0.0)
    z = dot_ref.fold(np.array([-0.0]))
    assert z == 0.0 and not np.signbit(z)  # the padding is added
    rng = np.random.default_rng(3)
    t = rng.standard_normal((5, 70000)) * np.exp(4 * rng.standard_normal((5, 70000)))
    got = dot_ref.fold(t)
    assert got.shape == (5,) and any(got[i] != dot_ref.running(t[i]) for i in range(5))
    two = dot_ref.fold(t[:, :65536]) + dot_ref.fold(t[:, 65536:])
    assert np.array_equal(got.view(np.uint64), two.view(np.uint64))  # the blocks are added in order


def test_the_quick_fold_is_the_stated_fold():
    """tests/dot_ref.py folds a short last block without its padding columns: the same bits as the definition word for word."""
    rng = np.random.default_rng(4)
    for m in (0, 1, 2, 3, 5, 255, 256, 257, 4097, 65535, 65536, 65537, 2 * 65536 + 3):
        t = rng.standard_normal((3, 2, m)) * np.exp(6 * rng.standard_normal((3, 2, m)))
        if m:
            t[0, 0, :] = -0.0  # only terms of -0.0: the padding decides the sign
            t[1, 1, : m // 2] = 0.0
        a, b = dot_ref.fold(t), dot_ref.fold_stated(t)
        assert a.shape == b.shape == (3, 2) and np.array_equal(a.view(np.uint64), b.view(np.uint64)), m
        if m and m % 65536:
            assert not np.signbit(a[0, 0])
