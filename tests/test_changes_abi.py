"""CPU-side checks of the change queries (dppr_mark, dppr_group_mark, dppr_unmark, dppr_group_unmark, dppr_changes,
dppr_group_changes): declared in include/dppr.h, exported by the library, listed in engine.EXPORTS, rejected without a handle;
and the result block of a call (dynamicppr_amd/csrc/dppr_changes_plan.hpp) driven by tests/native/changes_test.cpp under the
address and undefined-behaviour sanitizers. No GPU call is made."""
import ctypes
import os
import re
import subprocess

from dynamicppr_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_mark", "dppr_group_mark", "dppr_unmark", "dppr_group_unmark", "dppr_changes", "dppr_group_changes")


def header_text():
    return open(os.path.join(ROOT, "include", "dppr.h")).read()


def test_header_declares_the_six_calls_and_the_abi_is_still_6():
    text = header_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)  # backward compatible additions
    # the three calls that change a group's sources say that they drop the mark
    for name in ("dppr_group_replace_source", "dppr_group_add_source", "dppr_group_remove_source"):
        comment = re.findall(r"/\*((?:(?!\*/).)*?)\*/\s*int " + name + r"\s*\(", text, flags=re.S)
        assert comment and "mark" in comment[-1], name


def test_library_exports_the_calls():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    assert eng.lib().dppr_abi_version() == 6
    for name in ("mark", "group_mark", "unmark", "group_unmark", "changes", "group_changes"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ids = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    d = (ctypes.c_double * 4)(1.5, 1.5, 1.5, 1.5)
    p = (ctypes.c_double * 4)(2.5, 2.5, 2.5, 2.5)
    cnt, moved = ctypes.c_int32(-7), ctypes.c_int32(-9)
    for fn in (L.dppr_mark, L.dppr_group_mark, L.dppr_unmark, L.dppr_group_unmark):
        assert fn(None, 0) == -1
    assert L.dppr_changes(None, 0, 4, 0.0, 0, ids, d, p, ctypes.byref(cnt), ctypes.byref(moved)) == -1
    assert L.dppr_group_changes(None, 0, 4, 0.0, 1, ids, d, p, ctypes.byref(cnt), ctypes.byref(moved)) == -1
    assert list(ids) == [7] * 4 and list(d) == [1.5] * 4 and list(p) == [2.5] * 4 and cnt.value == -7 and moved.value == -9


def test_result_block_layout(tmp_path):
    """dppr_changes_plan.hpp: the sections of the result block are aligned, in order, disjoint and inside the block for every
    (n, k); what is copied back ends where the device-only section begins; the argument check equals its plain restatement."""
    exe = str(tmp_path / "changes_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "changes_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
