"""Top-k and point queries of a PPR state on the device (dppr_topk, dppr_group_topk, dppr_read_at, dppr_group_read_at)
against numpy over the dense reads: the same ids and the same bit patterns of p and r, for slots and groups of every row
width, ties, hand-written states (refinement, ulps, subnormals, negatives), parked vertices and invalid arguments."""
import ctypes as C

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_renumbering_gpu import churn_stream
from tests.util import small_stream

pytestmark = pytest.mark.gpu

KS = (1, 10, 1000, 8192)
EPS = 1e-9
MIN_PS = (0.0, EPS, 1e-4)


def expected(p, r, k, min_p):
    ids = np.nonzero(p > min_p)[0]
    order = np.lexsort((ids, -p[ids]))[:k]
    ids = ids[order]
    return ids.astype(np.int32), p[ids], r[ids]


def assert_same(got, p, r, k, min_p, what=""):
    gi, gp, gr = got
    wi, wp, wr = expected(p, r, k, min_p)
    assert np.array_equal(gi, wi), (what, k, min_p, gi[:8], wi[:8], len(gi), len(wi))
    assert np.array_equal(gp.view(np.uint64), wp.view(np.uint64)), (what, k, min_p)
    assert np.array_equal(gr.view(np.uint64), wr.view(np.uint64)), (what, k, min_p)


def check_slot(e, slot, ks=KS, min_ps=MIN_PS):
    p, r = e.read(slot)
    for k in ks:
        for mp in min_ps:
            assert_same(e.topk(slot, k, mp), p, r, k, mp, "slot")
    return p, r


def check_group(e, gid, n, ks=KS, min_ps=MIN_PS):
    dense = [e.group_read(gid, i) for i in range(n)]
    for k in ks:
        for mp in min_ps:
            res = e.group_topk(gid, k, mp)
            assert len(res) == n
            for i, (p, r) in enumerate(dense):
                assert_same(res[i], p, r, k, mp, f"group n={n} source {i}")
    return dense


@pytest.mark.parametrize("directed", [1, 0])
def test_solved_states_slot_and_groups_of_every_width(directed):
    V, e1, e2 = small_stream()
    W, c = 600, 20
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 16)]
    g = orc.Graph(V, e1, e2, directed, W, c)
    e = eng.Engine(V, W, directed, c)
    e.load_window(*g.window_edges())
    slot = e.add_source(srcs[0])
    groups = {n: e.add_source_group(srcs[:n]) for n in (1, 2, 3, 8, 10, 16)}
    e.init_solve(slot, EPS)
    for gid in groups.values():
        e.group_init_solve(gid, EPS)
    for b in range(3):
        if b:
            assert not g.stream_updates()
            g.inc_construct(1)
            e.set_batch(*g.batch())
            e.slide(*g.new_stream())
            e.update(slot, EPS)
            for gid in groups.values():
                e.group_update(gid, EPS)
        p, _ = check_slot(e, slot)
        assert 0 < np.count_nonzero(p > 0) < 8192  # (k = 8192 asks for more than qualify)
        for n, gid in groups.items():
            check_group(e, gid, n)


def test_ties_of_a_star_are_cut_in_external_id_order():
    """Leaves of a star are structurally identical: under the synchronous schedule their p are bit-identical. Leaves enter
    the stream in a shuffled order, so internal ids do not follow external ones; k cuts through the tie."""
    rng = np.random.default_rng(3)
    V, L = 4096, 300
    leaves = (rng.permutation(V - 1)[:L] + 1).astype(np.int32)
    assert not np.all(np.diff(leaves) > 0)
    e1, e2 = np.zeros(L, dtype=np.int32), leaves
    e = eng.Engine(V, L, 0, 1, schedule=eng.SCHEDULE_SYNC)
    e.load_window(e1, e2)
    slot = e.add_source(0)
    gid = e.add_source_group([0, int(leaves[5]), int(leaves[17])])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    p, r = e.read(slot)
    lv = p[leaves]
    assert np.all(lv.view(np.uint64) == lv[0].view(np.uint64)) and lv[0] > 0  # the tie exists
    assert p[0] > lv[0]
    for k in (1, 2, 40, L // 2 + 1, L, L + 1, 1000):
        assert_same(e.topk(slot, k), p, r, k, 0.0, "star")
    cut = e.topk(slot, 1 + 40)[0]
    assert cut[0] == 0 and np.array_equal(cut[1:], np.sort(leaves)[:40])  # k = 41 cuts the tie of 300
    check_group(e, gid, 3, ks=(1, 41, 301, 8192), min_ps=(0.0,))


def test_hand_written_states_through_write():
    """States set by dppr_write: a million values inside one exponent (the pass-1 bin overflows into the refinement, with
    ties among them), values one ulp apart, subnormals, negatives and -0.0 (never returned)."""
    V = 1 << 21
    rng = np.random.default_rng(7)
    e = eng.Engine(V, 2, 1, 1)
    e.load_window(np.array([0, 1], dtype=np.int32), np.array([1, 2], dtype=np.int32))
    slot = e.add_source(0)

    def run(p, r, ks=KS, min_ps=MIN_PS, what=""):
        e.write(slot, p, r)
        gp, gr = e.read(slot)
        assert np.array_equal(gp.view(np.uint64), p.view(np.uint64))
        for k in ks:
            for mp in min_ps:
                assert_same(e.topk(slot, k, mp), gp, gr, k, mp, what)

    ids = rng.permutation(V)[:1_000_000]
    p = np.zeros(V)
    p[ids] = 1.0 + rng.integers(0, 1 << 14, len(ids)) / float(1 << 14)  # [1, 2): one exponent, ~61 values per distinct p
    r = rng.standard_normal(V) * 1e-10
    run(p, r, what="one exponent")
    run(p, r, ks=(8192,), min_ps=(1.5, 1.9998,), what="one exponent, min_p inside it")

    p = np.zeros(V)
    vals = (np.full(20000, 0.3).view(np.uint64) + np.arange(20000, dtype=np.uint64)).view(np.float64)  # one ulp apart
    p[rng.permutation(V)[:20000]] = vals
    run(p, r, what="ulps")

    p = np.zeros(V)
    sub = rng.integers(1, 1 << 52, 5000, dtype=np.uint64).view(np.float64)  # subnormals
    sub[:100] = sub[100]  # (ties among them)
    p[rng.permutation(V)[:5000]] = sub
    run(p, r, ks=(1, 10, 5000, 8192), min_ps=(0.0, EPS), what="subnormals")

    p = np.zeros(V)
    at = rng.permutation(V)[:30000]
    p[at[:10000]] = -rng.random(10000)
    p[at[10000:20000]] = -0.0
    p[at[20000:]] = rng.random(10000) * 1e-3
    run(p, r, what="negatives and -0.0")
    got = e.topk(slot, 8192)[0]
    assert len(got) == 8192 and np.all(p[got] > 0)


def test_parked_vertices_are_found():
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    sources = [0, 1, 2]
    slot = e.add_source(0)
    gid = e.add_source_group(sources)
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    for _ in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.update(slot, EPS)
        e.group_update(gid, EPS)
    sp = e.id_space()
    assert sp["parked"] > 0 and sp["renumberings"] > 0, sp
    w1, w2 = g.window_edges()
    in_window = np.zeros(V, dtype=bool)
    in_window[w1] = in_window[w2] = True
    check_slot(e, slot, ks=(10, 1000, 8192))
    got = e.topk(slot, 8192)[0]
    assert np.any(~in_window[got])  # a parked vertex (no edge in the window) holds p > 0 and is returned
    check_group(e, gid, 3, ks=(10, 8192))
    for i in range(3):
        assert np.any(~in_window[e.group_topk(gid, 8192)[i][0]])


def test_point_reads_match_the_dense_reads():
    V, e1, e2 = small_stream()
    W, c = 600, 20
    rng = np.random.default_rng(5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.load_window(*g.window_edges())
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, 1, 10)]
    slot = e.add_source(srcs[0])
    groups = {n: e.add_source_group(srcs[:n]) for n in (1, 3, 10)}
    e.init_solve(slot, EPS)
    for gid in groups.values():
        e.group_init_solve(gid, EPS)
    p, r = e.read(slot)
    ids = rng.integers(0, V, 3000).astype(np.int32)
    never = np.setdiff1d(np.arange(V), np.concatenate([e1[:W], e2[:W], srcs]))
    assert len(never) > 0
    ids[:len(never[:50])] = never[:50]  # vertices that never had an internal id
    gp, gr = e.read_at(slot, ids)
    assert np.array_equal(gp.view(np.uint64), p[ids].view(np.uint64)) and np.array_equal(gr.view(np.uint64), r[ids].view(np.uint64))
    assert np.all(gp[:len(never[:50])] == 0.0)
    for n, gid in groups.items():
        ap, ar = e.group_read_at(gid, ids)
        assert ap.shape == (len(ids), n)
        for i in range(n):
            dp, dr = e.group_read(gid, i)
            assert np.array_equal(ap[:, i].view(np.uint64), dp[ids].view(np.uint64))
            assert np.array_equal(ar[:, i].view(np.uint64), dr[ids].view(np.uint64))
    empty = e.read_at(slot, np.zeros(0, dtype=np.int32))
    assert len(empty[0]) == 0


def test_invalid_arguments_are_rejected_and_nothing_is_written():
    V, e1, e2 = small_stream()
    W, c = 600, 20
    e = eng.Engine(V, W, 1, c)
    e.load_window(e1[:W], e2[:W])
    slot = e.add_source(int(e1[0]))
    gid = e.add_source_group([int(e1[0]), int(e2[0])])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    L, h = eng.lib(), e._h
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    K = 16
    ids = np.full(2 * K, 77, dtype=np.int32)
    pv = np.full(2 * K, 3.25)
    rv = np.full(2 * K, 4.5)
    cnt = np.full(2, 99, dtype=np.int32)
    I, P, R, N = ids.ctypes.data_as(ip), pv.ctypes.data_as(dp), rv.ctypes.data_as(dp), cnt.ctypes.data_as(ip)

    def untouched():
        return np.all(ids == 77) and np.all(pv == 3.25) and np.all(rv == 4.5) and np.all(cnt == 99)

    bad = [(slot, 0, 0.0, I, P, R, N), (slot, 8193, 0.0, I, P, R, N), (slot, -1, 0.0, I, P, R, N),
           (slot, K, -1e-300, I, P, R, N), (slot, K, float("nan"), I, P, R, N), (slot, K, 0.0, None, P, R, N),
           (slot, K, 0.0, I, None, R, N), (slot, K, 0.0, I, P, R, None)]
    for a in bad:
        assert L.dppr_topk(h, *a) == -1, a
        assert untouched(), a
    assert L.dppr_topk(h, 5, K, 0.0, I, P, R, N) == -1 and untouched()
    for a in bad:
        assert L.dppr_group_topk(h, gid, *a[1:]) == -1, a
        assert untouched(), a
    assert L.dppr_group_topk(h, 3, K, 0.0, I, P, R, N) == -1 and untouched()
    for wrong in ([0, -1], [V, 0], [1, V + 5]):
        q = np.array(wrong, dtype=np.int32)
        assert L.dppr_read_at(h, slot, q.ctypes.data_as(ip), 2, P, R) == -1 and untouched()
        assert L.dppr_group_read_at(h, gid, q.ctypes.data_as(ip), 2, P, R) == -1 and untouched()
    q = np.array([0, 1], dtype=np.int32)
    assert L.dppr_read_at(h, 9, q.ctypes.data_as(ip), 2, P, R) == -1 and untouched()
    assert L.dppr_group_read_at(h, 9, q.ctypes.data_as(ip), 2, P, R) == -1 and untouched()
    assert L.dppr_read_at(h, slot, None, 2, P, R) == -1 and untouched()
    assert L.dppr_read_at(h, slot, q.ctypes.data_as(ip), -1, P, R) == -1 and untouched()
    # and a valid call afterwards writes exactly the documented shape: count, then -1 / 0.0 past it
    assert L.dppr_topk(h, slot, K, 1e300, I, P, None, N) == 0
    assert cnt[0] == 0 and np.all(ids[:K] == -1) and np.all(pv[:K] == 0.0) and np.all(rv == 4.5) and np.all(ids[K:] == 77)
