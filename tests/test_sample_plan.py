"""CPU-side checks of the sampling queries (dppr_sample, dppr_group_sample): declared in include/dppr.h with their contract,
exported by the library, listed in engine.EXPORTS with their prototypes, rejected without a handle with nothing written; the
HIP-free plan and THE definition of a draw (dynamicppr_amd/csrc/dppr_sample_plan.hpp) driven by tests/native/sample_plan_test.cpp
as a stand-alone program under the address and undefined-behaviour sanitizers; the refusals of ./pagerank --sample; the numpy
reference (tests/sample_ref.py) on a case worked out by hand and on its statistics. No GPU call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from dynamicppr_amd import engine as eng
from tests import sample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dppr_sample", "dppr_group_sample", "dppr_debug_sample_form")


def test_header_declares_the_calls_and_the_abi_is_still_6():
    text = open(os.path.join(ROOT, "include", "dppr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert re.search(r"^#define DPPR_ABI_VERSION 6\b", text, re.M)
    for name, value in (("DPPR_SAMPLE_MAX", r"\(1 << 20\)"), ("DPPR_SAMPLE_MAX_TOTAL", r"\(1 << 24\)"), ("DPPR_SAMPLE_OK", "0"), ("DPPR_SAMPLE_EMPTY", "1"),
                        ("DPPR_SAMPLE_NONFINITE", "2")):
        assert re.search(r"^#define " + name + r"\s+" + value + r"\s*$", code, re.M), name
    assert (eng.SAMPLE_MAX, eng.SAMPLE_MAX_TOTAL) == (1 << 20, 1 << 24) and (eng.SAMPLE_OK, eng.SAMPLE_EMPTY, eng.SAMPLE_NONFINITE) == (0, 1, 2)
    # the contract is stated where a caller reads it
    for phrase in ("THE SCORE of dppr_topk_ranked", "w_i[v] = +0.0", "smallest power of two >= V", "EXTERNAL id", "y[j] = y_l[2j] + y_l[2j + 1], one rounding",
                   "number of\n *    positive leaves", "DPPR_SAMPLE_EMPTY", "DPPR_SAMPLE_NONFINITE", "0x53414D50", "(lo32 seed, hi32 seed)",
                   ">> 11) * 2^-53", "x = u * root, one rounding", "if x >= L and R > 0 then x = x - L", "only ever enters a node of positive value",
                   "its own leaves, its lane index, seed and j alone", "The contract is\n * the definition", "log2(P) * 2^-52",
                   "equal to out_w bit for bit", "followed by those of (first + a, b)", "returns it S times", "S == 0 is valid",
                   "first + S wrapping", "obtained before the first kernel", "OUT OF SCOPE", "without replacement", "alias tables",
                   "do\n * not depend on the form"):
        assert phrase in text, phrase


def test_library_exports_the_calls_with_their_prototypes():
    lib = ctypes.CDLL(eng.build())
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in eng.EXPORTS
    L = eng.lib()
    assert L.dppr_abi_version() == 6
    for fn in (L.dppr_sample, L.dppr_group_sample):
        assert len(fn.argtypes) == 14 and fn.restype is ctypes.c_int
        assert fn.argtypes[4] is ctypes.c_double and fn.argtypes[5] is ctypes.c_uint64 and fn.argtypes[6] is ctypes.c_uint64
        assert fn.argtypes[7] is ctypes.c_int32 and fn.argtypes[8] is ctypes.c_int
    assert len(L.dppr_debug_sample_form.argtypes) == 2
    for name in ("sample", "group_sample", "group_sample_dev", "debug_sample_form"):
        assert callable(getattr(eng.Engine, name)), name


def test_invalid_handle_is_rejected_without_a_device():
    L = eng.lib()
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    ids, w = np.full(4, 7, dtype=np.int32), np.full(4, 2.5)
    total, support, status = np.full(1, 2.5), np.full(1, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    for fn in (L.dppr_sample, L.dppr_group_sample):
        assert fn(None, 0, -1, None, 0.0, 1, 0, 4, eng.DEST_HOST, ids.ctypes.data, w.ctypes.data, total.ctypes.data_as(dp), support.ctypes.data_as(ip),
                  status.ctypes.data_as(ip)) == -1
    assert L.dppr_debug_sample_form(None, 0) == -1
    assert np.all(ids == 7) and np.all(w == 2.5) and np.all(total == 2.5) and np.all(support == 7) and np.all(status == 7)


def test_sample_plan(tmp_path):
    """dppr_sample_plan.hpp: level offsets that do not overlap and are aligned for V in {1, 2, 255, 256, 257, 2047, 2048, 2049,
    65 536, 65 537} and n in {1, 10, 16}, every argument rule at its limit, the uniform at both ends, the descent against a linear
    scan on exact dyadic weights, the step never entering a zero node over 10^5 random trees."""
    exe = str(tmp_path / "sample_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "sample_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_cli_refuses_bad_sample_flags(tmp_path):
    """--sample 0, a negative value, a value above DPPR_SAMPLE_MAX, --sample with --split, and --sample-seed without --sample:
    invalid arguments and the usage, before any device work."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    srcs = str(tmp_path / "sources.txt")
    open(srcs, "w").write("1\n2\n3\n4\n")
    base = [BIN, "-d", path, "-a", "0", "-i", "1", "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", "2", "--sources", srcs]
    for bad in (["--sample", "0"], ["--sample", "-5"], ["--sample", str(eng.SAMPLE_MAX + 1)], ["--sample-seed", "7"], ["--sample", "64", "--split"],
                ["--sample", "64", "--rank-factor", "nonsense"]):
        r = run(base + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and "--sample <S> [--sample-seed <X>]" in r.stdout, (bad, r.stdout[-400:])
        assert "start..." not in r.stdout and "no CPU fallback" not in r.stdout, (bad, r.stdout[-400:])


def test_reference_on_a_hand_computed_case():
    """Five vertices. Every number below was worked out by hand from the definition of include/dppr.h: the leaves are padded to
    eight, the pairs give [0.5, 0.375, 0.125, 0], then [0.875, 0.125], the root is 1.0."""
    w = np.array([0.5, 0.0, 0.25, 0.125, 0.125])
    lv = ref.tree(w)
    assert [l.tolist() for l in lv] == [[0.5, 0.0, 0.25, 0.125, 0.125, 0.0, 0.0, 0.0], [0.5, 0.375, 0.125, 0.0], [0.875, 0.125], [1.0]]
    # 0.6: left at the root (0.6 < 0.875), right of 0.5 with x = 0.1 (exactly 0.6 - 0.5), left of 0.25: leaf 2
    assert ref.descend(lv, [0.6]).tolist() == [2]
    # 0.8: left, right with x = 0.8 - 0.5, then 0.3 >= 0.25: right: leaf 3
    assert ref.descend(lv, [0.8]).tolist() == [3]
    # 0.9 and 0.95 take the right branch at the root; below it the right sibling is +0.0 twice, so both go left twice: leaf 4
    assert ref.descend(lv, [0.9, 0.95]).tolist() == [4, 4]
    # x >= L and R == 0 must go left: x = 0.124 below the root's right child stays in leaf 4, never in the padding leaf 5
    assert ref.descend(lv, [0.875 + 0.124, 0.875]).tolist() == [4, 4]
    # x rounded up to the root itself: right wherever the right child is positive, ending on the last positive leaf
    assert ref.descend(lv, [1.0]).tolist() == [4]
    u = 1.0 - 2.0 ** -53
    tiny = ref.tree(np.array([2.0 ** -1074, 0.0, 2.0 ** -1074]))
    assert u * tiny[-1][0] == tiny[-1][0] and ref.descend(tiny, [u * tiny[-1][0]]).tolist() == [2]
    # the left edge of a leaf belongs to it; zero-weight leaves are never drawn
    assert ref.descend(lv, [0.0, 0.49, 0.5, 0.75, 0.87]).tolist() == [0, 0, 2, 3, 3]
    # weights: NaN, negatives, zeros and scores at or below the threshold weigh +0.0
    got = ref.weights(np.array([0.5, -1.0, np.nan, 0.0, -0.0, 1e-4, np.inf]), 1e-4)
    assert got.tolist() == [0.5, 0.0, 0.0, 0.0, 0.0, 0.0, np.inf] and not np.signbit(got).any()
    assert ref.status(0.0) == ref.EMPTY and ref.status(np.inf) == ref.NONFINITE and ref.status(1e-300) == ref.OK
    ids, ww = ref.draw(ref.tree(np.zeros(3)), 0, 1, 0, 5)
    assert ids.tolist() == [-1] * 5 and ww.tolist() == [0.0] * 5
    # the uniforms: 53 bits in [0, 1), a function of (lane, seed, draw number) that crosses the 32-bit counter word
    a = ref.uniforms(3, 99, 2 ** 32 - 3, 6)
    assert np.all((a >= 0) & (a < 1)) and np.array_equal(a[3:], ref.uniforms(3, 99, 2 ** 32, 3)) and not np.array_equal(a[:3], ref.uniforms(3, 99, 2 ** 32, 3))
    assert np.all(a * 2.0 ** 53 == np.floor(a * 2.0 ** 53))
    assert not np.array_equal(ref.uniforms(2, 99, 0, 6), ref.uniforms(3, 99, 0, 6)) and not np.array_equal(ref.uniforms(3, 98, 0, 6), ref.uniforms(3, 99, 0, 6))


def test_reference_statistics():
    """2^18 draws over 300 positive weights spanning six orders of magnitude, with zeros between them: every vertex's frequency
    within 5 sqrt(q (1 - q) / N) of q = w / total, no zero-weight vertex drawn. Deterministic: one committed seed.

    The layout of the weights is by reasoning, not by outcome. The bound is a Gaussian one, and with N = 2^18 a vertex of
    q < 1 / (25 N) = 1.5e-7 misses it by being drawn ONCE: its count is Poisson, not normal. Log-uniform weights (total about 21,
    q down to 5e-8) put some 27 vertices there with 0.5 expected draws among them, so a CORRECT sampler misses the bound in four
    runs of ten. The layout below keeps every magnitude 10^0 .. 10^-6 present (each weight times a factor in [1, 1.5)) but most
    of the mass in few vertices -- 1, 9, 270, 5, 5, 5, 5 per magnitude, total about 5.8 --, so the smallest q is about 1.7e-7, a
    single draw of any vertex is inside its bound, and the Poisson tails beyond the bounds sum to about 1 % over all vertices."""
    rng = np.random.default_rng(2024)
    V, N = 1000, 1 << 18
    w = np.zeros(V)
    pos = np.sort(rng.permutation(V)[:300])
    mags = np.concatenate([np.full(c, 10.0 ** -m) for m, c in enumerate((1, 9, 270, 5, 5, 5, 5))])
    w[pos] = rng.permutation(mags) * (1.0 + 0.5 * rng.random(300))
    assert w[pos].max() / w[pos].min() >= 1e6 / 1.5
    lv = ref.tree(w)
    total = lv[-1][0]
    ids, ww = ref.draw(lv, 4, 20240607, 0, N)
    assert np.all(w[ids] > 0) and np.array_equal(ww, w[ids])
    freq = np.bincount(ids, minlength=V) / N
    q = w / total
    bound = 5.0 * np.sqrt(q * (1.0 - q) / N)
    assert np.all(1.0 / N - q[pos] <= bound[pos])        # (one draw of a vertex is inside its bound: see above)
    worst = np.max(np.abs(freq - q)[pos] / bound[pos])
    assert np.all(np.abs(freq - q) <= bound), worst
    assert np.all(freq[w == 0] == 0)
