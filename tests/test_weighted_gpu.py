"""A source group queried as a weighted set of targets (dppr_group_topk_weighted, dppr_group_score_at) against numpy over the
dense reads. The reference is the fold of include/dppr.h as a Python loop over the columns of group_read (numpy's multiply and
add are separate roundings, nothing fused), `score > min_score` as the filter and np.lexsort((ids, -score)) as the order; ids are
compared with array_equal and scores by their bit patterns."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_renumbering_gpu import churn_stream
from tests.util import small_stream

pytestmark = pytest.mark.gpu

KS = (1, 10, 1000, 8192)
EPS = 1e-9
MIN_SCORES = (0.0, EPS, 1e-4)
WIDTHS = (1, 2, 3, 8, 9, 10, 16)  # narrow and wide rows, the padding lane, the 8 -> 9 switch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def fold(cols, w):
    """The score of include/dppr.h: cols[i] is column i (any shape), w one weight vector."""
    acc = w[0] * cols[0]
    for i in range(1, len(cols)):
        acc = acc + w[i] * cols[i]
    return acc


def expected(score, k, min_score):
    ids = np.nonzero(score > min_score)[0]
    ids = ids[np.lexsort((ids, -score[ids]))[:k]]
    return ids.astype(np.int32), score[ids]


def weight_sets(n, rng):
    mixed = rng.standard_normal((16, n))
    mixed[rng.random((16, n)) < 0.2] = 0.0  # some exact zeros
    mixed[0, 0] = 0.0
    return [np.ones((1, n)), rng.random((3, n)), mixed]


def check_weighted(e, gid, n, w, ks=KS, min_scores=MIN_SCORES, cols=None):
    """Every weight vector of w ([q][n]) for every k and min_score; returns the dense columns and the result lengths seen."""
    cols = cols if cols is not None else [e.group_read(gid, i)[0] for i in range(n)]
    scores = [fold(cols, wj) for wj in w]
    lengths = []
    for k in ks:
        for ms in min_scores:
            res = e.group_topk_weighted(gid, w, k, ms)
            assert len(res) == len(w)
            for j, (gi, gs) in enumerate(res):
                wi, ws = expected(scores[j], k, ms)
                assert np.array_equal(gi, wi), (n, j, k, ms, gi[:8], wi[:8], len(gi), len(wi))
                assert np.array_equal(bits(gs), bits(ws)), (n, j, k, ms)
                lengths.append((k, len(gi)))
    return cols, lengths


def star(L, sources_of, V=4096, seed=3):
    """The star of tests/test_topk_gpu.py: L leaves that enter the stream in a shuffled order, synchronous schedule."""
    rng = np.random.default_rng(seed)
    leaves = (rng.permutation(V - 1)[:L] + 1).astype(np.int32)
    assert not np.all(np.diff(leaves) > 0)
    e = eng.Engine(V, L, 0, 1, schedule=eng.SCHEDULE_SYNC)
    e.load_window(np.zeros(L, dtype=np.int32), leaves)
    sources = sources_of(leaves)
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, EPS)
    return e, gid, leaves, sources


class Solved:
    """An engine over the small stream with one group per width, after the init solve and after later updates."""

    def __init__(self, directed, widths=WIDTHS, W=600, c=20):
        V, e1, e2 = small_stream()
        self.V, self.e1, self.e2, self.W = V, e1, e2, W
        self.srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 16)]
        self.g = orc.Graph(V, e1, e2, directed, W, c)
        self.e = eng.Engine(V, W, directed, c)
        self.e.load_window(*self.g.window_edges())
        self.groups = {n: self.e.add_source_group(self.srcs[:n]) for n in widths}
        for gid in self.groups.values():
            self.e.group_init_solve(gid, EPS)

    def update(self, batches):
        for _ in range(batches):
            assert not self.g.stream_updates()
            self.g.inc_construct(1)
            self.e.set_batch(*self.g.batch())
            self.e.slide(*self.g.new_stream())
            for gid in self.groups.values():
                self.e.group_update(gid, EPS)


@pytest.mark.parametrize("directed", [1, 0])
def test_every_row_width(directed):
    s = Solved(directed)
    rng = np.random.default_rng(11)
    short = 0
    for state in ("init", "two updates"):
        if state != "init":
            s.update(2)
        for n, gid in s.groups.items():
            cols = None
            for w in weight_sets(n, rng):
                cols, lengths = check_weighted(s.e, gid, n, w, cols=cols)
                short += sum(1 for k, got in lengths if got < k)
    assert short > 0  # (k = 8192 asks for more than qualify)
    s.e.close()


@pytest.mark.parametrize("directed", [1, 0])
def test_one_hot_weights_equal_group_topk(directed):
    s = Solved(directed)
    s.update(1)
    for n, gid in s.groups.items():
        for k in (10, 8192):
            for ms in (0.0, 1e-4):
                plain = s.e.group_topk(gid, k, ms)
                got = s.e.group_topk_weighted(gid, np.eye(n), k, ms)
                assert len(got) == len(plain) == n
                for i in range(n):
                    assert np.array_equal(got[i][0], plain[i][0]), (n, i, k, ms)
                    assert np.array_equal(bits(got[i][1]), bits(plain[i][1])), (n, i, k, ms)
    s.e.close()


def test_ties_are_cut_in_external_id_order():
    L = 300
    e, gid, leaves, sources = star(L, lambda lv: [0, int(lv[5]), int(lv[17])])
    w = np.array([[1.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    cols = [e.group_read(gid, i)[0] for i in range(3)]
    # the tie exists in the numpy scores: every leaf under (1, 0, 0), every leaf but the two sources under (1, 1, 1)
    s0, s1 = fold(cols, w[0]), fold(cols, w[1])
    assert len(np.unique(bits(s0[leaves]))) == 1 and 0 < s0[leaves[0]] < s0[0]
    others = np.setdiff1d(leaves, sources[1:])
    assert len(others) == L - 2 and len(np.unique(bits(s1[others]))) == 1 and s1[others[0]] > 0
    check_weighted(e, gid, 3, w, ks=(2, 41, 151, 300, 301, 1000), min_scores=(0.0,), cols=cols)
    cut = e.group_topk_weighted(gid, w[0], 41)[0][0]
    assert cut[0] == 0 and np.array_equal(cut[1:], np.sort(leaves)[:40])  # k = 41 cuts the tie of 300
    e.close()


@pytest.mark.parametrize("L", [510, 511, 512])
def test_chunk_edges(L):
    """L + 1 occupied rows around the 512 rows of a chunk of the streaming passes (and 4 tiles of the score kernel)."""
    e, gid, leaves, sources = star(L, lambda lv: [0, int(lv[0])])
    sp = e.id_space()
    assert sp["ids"] + sp["parked"] == L + 1
    w = np.array([[1.0, 1.0], [0.25, -0.5]])
    _, lengths = check_weighted(e, gid, 2, w, ks=(1, 8192), min_scores=(0.0,))
    assert (8192, L + 1) in lengths  # all ones: every occupied row qualifies
    e.close()


def test_parked_zone_is_scanned():
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    gid = e.add_source_group([0, 1, 2])
    e.group_init_solve(gid, EPS)
    for _ in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.group_update(gid, EPS)
    sp = e.id_space()
    assert sp["parked"] > 0 and sp["renumberings"] > 0, sp
    w1, w2 = g.window_edges()
    in_window = np.zeros(V, dtype=bool)
    in_window[w1] = in_window[w2] = True
    w = np.array([[1.0, 1.0, 1.0], [0.5, -0.25, 2.0]])
    check_weighted(e, gid, 3, w, ks=(10, 8192), min_scores=(0.0,))
    got = e.group_topk_weighted(gid, w[0], 8192)[0][0]
    assert np.any(~in_window[got])  # a parked vertex (no edge in the window) holds a score > 0 and is returned
    e.close()


def test_score_at_matches_the_fold_over_the_point_reads():
    s = Solved(1, widths=(1, 3, 10))
    rng = np.random.default_rng(5)
    V = s.V
    ids = rng.integers(0, V, 3000).astype(np.int32)
    never = np.setdiff1d(np.arange(V), np.concatenate([s.e1[:s.W], s.e2[:s.W], s.srcs]))[:50]
    assert len(never) == 50
    ids[:50] = never  # vertices that never had an internal id
    for n, gid in s.groups.items():
        p_at, _ = s.e.group_read_at(gid, ids)
        assert np.all(p_at[:50] == 0.0)
        for q in (1, 16):
            w = rng.standard_normal((q, n))
            w[0] = -np.abs(w[0]) - 0.5  # (an id-less vertex under negative weights scores -0.0: every term is -0.0)
            got = s.e.group_score_at(gid, w, ids)
            assert got.shape == (len(ids), q)
            for j in range(q):
                want = fold([p_at[:, i] for i in range(n)], w[j])
                assert np.array_equal(bits(got[:, j]), bits(want)), (n, q, j)
            assert np.all(np.signbit(got[:50, 0])) and np.all(got[:50, 0] == 0.0)
        empty = s.e.group_score_at(gid, np.ones(n), np.zeros(0, dtype=np.int32))
        assert empty.shape == (0, 1)
    s.e.close()


def test_the_query_follows_added_and_removed_sources():
    s = Solved(1, widths=(3,))
    gid = s.groups[3]
    rng = np.random.default_rng(9)
    idx, _ = s.e.group_add_source(gid, s.srcs[5])
    assert idx == 3 and s.e.group_sources(gid) == s.srcs[:3] + [s.srcs[5]]
    check_weighted(s.e, gid, 4, rng.standard_normal((3, 4)), ks=(10, 8192), min_scores=(0.0, 1e-4))
    s.e.group_remove_source(gid, 0)
    assert s.e.group_sources(gid) == s.srcs[1:3] + [s.srcs[5]]
    w = rng.standard_normal((2, 3))
    cols, _ = check_weighted(s.e, gid, 3, w, ks=(10, 8192), min_scores=(0.0, 1e-4))
    one_hot = s.e.group_topk_weighted(gid, [0.0, 0.0, 1.0], 5)[0]  # the last lane is the added source
    assert one_hot[0][0] == s.srcs[5]
    ids = np.arange(s.V, dtype=np.int32)
    assert np.array_equal(bits(s.e.group_score_at(gid, w[0], ids)[:, 0]), bits(fold(cols, w[0])))
    with pytest.raises(eng.DpprError):
        s.e.group_topk_weighted(gid, np.ones(4), 5)  # the old width
    s.e.close()


def test_invalid_arguments_are_rejected_and_nothing_is_written():
    V, e1, e2 = small_stream()
    W, c = 600, 20
    e = eng.Engine(V, W, 1, c)
    e.load_window(e1[:W], e2[:W])
    gid = e.add_source_group([int(e1[0]), int(e2[0])])
    e.group_init_solve(gid, EPS)
    L, h = eng.lib(), e._h
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    K, Q = 16, 2
    ids = np.full(3 * K, 77, dtype=np.int32)
    sc = np.full(3 * K, 3.25)
    cnt = np.full(3, 99, dtype=np.int32)
    I, S, N = ids.ctypes.data_as(ip), sc.ctypes.data_as(dp), cnt.ctypes.data_as(ip)

    def wp(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        wp.keep.append(a)
        return a.ctypes.data_as(dp)
    wp.keep = []

    def untouched():
        return np.all(ids == 77) and np.all(sc == 3.25) and np.all(cnt == 99)

    good = wp(np.ones((Q, 2)))
    many = wp(np.ones((17, 2)))
    bad = [(gid, good, 0, K, 0.0, I, S, N), (gid, many, 17, K, 0.0, I, S, N), (gid, good, -1, K, 0.0, I, S, N),
           (gid, good, Q, 0, 0.0, I, S, N), (gid, good, Q, 8193, 0.0, I, S, N), (gid, good, Q, -1, 0.0, I, S, N),
           (gid, good, Q, K, -1e-300, I, S, N), (gid, good, Q, K, float("nan"), I, S, N),
           (gid, wp([[1.0, float("nan")], [1.0, 1.0]]), Q, K, 0.0, I, S, N),
           (gid, wp([[1.0, 1.0], [float("inf"), 1.0]]), Q, K, 0.0, I, S, N),
           (gid, wp([[1.0, 1.0], [1.0, -float("inf")]]), Q, K, 0.0, I, S, N),
           (gid, None, Q, K, 0.0, I, S, N), (gid, good, Q, K, 0.0, None, S, N), (gid, good, Q, K, 0.0, I, None, N),
           (gid, good, Q, K, 0.0, I, S, None), (3, good, Q, K, 0.0, I, S, N), (-1, good, Q, K, 0.0, I, S, N)]
    for a in bad:
        assert L.dppr_group_topk_weighted(h, *a) == -1, a
        assert untouched(), a
    at = np.array([0, 1], dtype=np.int32)
    A = at.ctypes.data_as(ip)
    bad_at = [(gid, good, 0, A, 2, S), (gid, many, 17, A, 2, S), (gid, None, Q, A, 2, S),
              (gid, wp([[1.0, float("nan")], [1.0, 1.0]]), Q, A, 2, S), (gid, wp([[float("inf"), 0.0], [1.0, 1.0]]), Q, A, 2, S),
              (gid, good, Q, None, 2, S), (gid, good, Q, A, -1, S), (gid, good, Q, A, 2, None), (9, good, Q, A, 2, S)]
    for wrong in ([0, -1], [V, 0], [1, V + 5]):
        q = np.array(wrong, dtype=np.int32)
        wp.keep.append(q)
        bad_at.append((gid, good, Q, q.ctypes.data_as(ip), 2, S))
    for a in bad_at:
        assert L.dppr_group_score_at(h, *a) == -1, a
        assert untouched(), a
    assert L.dppr_group_score_at(h, gid, good, Q, None, 0, S) == 0 and untouched()  # m == 0: a valid no-op
    # and a valid call afterwards writes exactly the documented shape: counts, then -1 / 0.0 past them, nothing beyond [q][k]
    assert L.dppr_group_topk_weighted(h, gid, good, Q, K, 1e300, I, S, N) == 0
    assert np.all(cnt[:Q] == 0) and cnt[Q] == 99
    assert np.all(ids[:Q * K] == -1) and np.all(sc[:Q * K] == 0.0) and np.all(ids[Q * K:] == 77) and np.all(sc[Q * K:] == 3.25)
    e.close()


def test_every_buffer_goes_with_the_engine():
    gc.collect()
    before = eng.live_bytes()
    s = Solved(1, widths=(10,))
    held = eng.live_bytes()
    rng = np.random.default_rng(2)
    res = s.e.group_topk_weighted(s.groups[10], rng.standard_normal((16, 10)), 8192)
    assert len(res) == 16 and any(len(ids) for ids, _ in res)
    s.e.group_score_at(s.groups[10], np.ones(10), np.arange(s.V, dtype=np.int32))
    assert eng.live_bytes()[0] > held[0]  # (the scratch state and the weights are there)
    s.e.close()
    assert eng.live_bytes() == before
