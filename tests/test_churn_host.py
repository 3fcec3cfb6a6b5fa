"""Width and lane planning of a source group that changes its sources (dynamicppr_amd/csrc/dppr_churn_plan.hpp, HIP-free): driven on
the CPU by tests/native/churn_test.cpp for every source count 1..16, every operation and index, against a plain restatement; built
with the address and undefined-behaviour sanitizers. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_churn_plan_equals_its_plain_restatement(tmp_path):
    """New n, gw == row_width(n') and spl; the column map is the surviving lanes in order, padding and new lanes map to -1; the
    relayout and re-cut flags."""
    exe = str(tmp_path / "churn_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "churn_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
