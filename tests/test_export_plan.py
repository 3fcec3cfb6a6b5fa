"""CPU-side checks of the exports (dppr_support, dppr_export_sparse, dppr_export_dense_dev and their group forms): declared in
include/dppr.h, exported by the library, listed in engine.EXPORTS, rejected without a handle with nothing written; and the
HIP-free plan of a call (dynamicppr_amd/csrc/dppr_export_plan.hpp) driven by tests/native/export_plan_test.cpp as a stand-alone
program under the address and undefined-behaviour sanitizers. No GPU call is made."""
import ctypes
import os
import re
import subprocess

from dynamicppr_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_support", "dppr_group_support", "dppr_export_sparse", "dppr_group_export_sparse", "dppr_export_dense_dev",
         "dppr_group_export_dense_dev")


def test_header_declares_the_six_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, value in (("DPPR_DEST_HOST", 0), ("DPPR_DEST_DEVICE", 1), ("DPPR_DENSE_P", 0), ("DPPR_DENSE_R", 1), ("DPPR_F64", 0),
                        ("DPPR_F32", 1), ("DPPR_VERTEX_MAJOR", 0), ("DPPR_SOURCE_MAJOR", 1)):
        assert re.search(rf"^#define {name} {value}\b", code, re.M), name
    assert (eng.DEST_HOST, eng.DEST_DEVICE, eng.DENSE_P, eng.DENSE_R, eng.F64, eng.F32, eng.VERTEX_MAJOR, eng.SOURCE_MAJOR) == (0, 1, 0, 1, 0, 1, 0, 1)


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("support", "group_support", "export_sparse", "group_export_sparse", "export_sparse_dev", "group_export_sparse_dev",
                 "export_dense_dev", "group_export_dense_dev"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    off = (ctypes.c_int64 * 3)(-7, -7, -7)
    ids = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    p = (ctypes.c_double * 4)(2.5, 2.5, 2.5, 2.5)
    A = ctypes.addressof
    assert L.dppr_support(None, 0, 0.0, off) == -1 and L.dppr_group_support(None, 0, 0.0, off) == -1
    for fn in (L.dppr_export_sparse, L.dppr_group_export_sparse):
        assert fn(None, 0, 0.0, 4, eng.DEST_HOST, off, A(ids), A(p), None) == -1
    assert L.dppr_export_dense_dev(None, 0, 0, 0, A(p)) == -1
    assert L.dppr_group_export_dense_dev(None, 0, 0, 0, 0, A(p)) == -1
    assert list(off) == [-7] * 3 and list(ids) == [7] * 4 and list(p) == [2.5] * 4


def test_export_plan(tmp_path):
    """dppr_export_plan.hpp: tile counts, workspace and block sizes, the bytes / alignment / indices of a dense destination for every
    (dtype, layout, n 1-16, V in {1, 255, 256, 257, 2^22}), 64-bit sizes beyond 2^31, the range check and the argument checks."""
    exe = str(tmp_path / "export_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "export_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]

