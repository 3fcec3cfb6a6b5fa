"""Chunk and launch policy of the frontier loops (dynamicppr_amd/csrc/dppr_loop_plan.hpp, HIP-free): driven on the CPU by
tests/native/loop_plan_test.cpp against a plain restatement of the expressions the loops held inline before -- every combination of
the small inputs, seeded random large ones, and whole loops replayed (decaying frontiers with and without a plateau, a push tail that
gives up, one whose lists overflow). One layer above the loops: the outcome of a whole-batch launch (ahead_outcome, apply_ahead) against
the transcribed tail of batch_ahead -- all sixteen combinations of the four status bits, stop positions 0, 1, 2, n-1, n, n+1 of logs of 1
to 128 entries with no zero, a zero in every position in turn (a leading one included), two adjacent zeros and random ones, cnt[4] 0 / 1,
merged x inline update x grouped; every output field and every mutated history, start_dense, last_F0 and statistics word -- and what a
batch runs after it (after_launch) against the transcribed body of dppr_update, for every outcome the former produces and without a
launch. Which representation of a single-source loop's frontier is live (FrontierForm: list, dense snapshot, extracted, any sweep ran, x left
clean) against the loop's former loose flags over every sequence of up to six events it can enqueue, from a loop's start and from a resumed
one, with the combinations the loop relies on asserted. Built with the address and undefined-behaviour sanitizers. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loop_plan_equals_its_plain_restatement(tmp_path):
    """Chunk sizes, thresholds, launch allowances, the push-or-sweep decision and its running means, the split of a whole-batch
    launch's log, and the histories element for element; a history saved and put back around a loop is bit-equal to before; the outcome
    of a whole-batch launch, what it leaves in the slot and the steps a batch runs after it, each equal to the code they replaced."""
    exe = str(tmp_path / "loop_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "loop_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
