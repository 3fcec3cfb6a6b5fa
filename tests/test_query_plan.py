"""CPU-side check of what the state queries share before any device is involved (dynamicppr_amd/csrc/dppr_query_plan.hpp): the result
block of a top-k call, the buffer of the point reads, the id range check and the argument checks of top-k, the point reads and the
weighted forms, driven by tests/native/query_plan_test.cpp as a stand-alone program under the address and undefined-behaviour
sanitizers. No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_plan(tmp_path):
    """dppr_query_plan.hpp: the top-k block for n 1-16 x k in {1, 2, 3, 100, 8191, 8192} x with / without r (offsets, alignment, copy
    and total bytes, the first-use allocation), the read_at / score_at buffers for m in {1, 2, 3, 4096}, ids_in_range at the edges of
    [0, V) and at m = 0, topk_args_ok, read_at_args_ok and weights_ok against plain restatements."""
    exe = str(tmp_path / "query_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "query_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
