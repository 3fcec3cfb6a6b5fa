"""The conductance sweep over a top-k order on the device (dppr_cluster / dppr_group_cluster) against the numpy restatement of
tests/cluster_ref.py over what the engine reports through its other calls: the order from topk / group_topk, the rows from
read_out_graph, Ed from the same epoch. Every output is compared exactly; best_phi by bit pattern."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import cluster_ref
from tests.cf_stream import conflict_free_stream
from tests.test_changes_gpu import bits
from tests.test_cluster_plan import planted_partition
from tests.test_conflict_free_streams import EPS as CF_EPS, SMALL
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 63, 64, 65, 1000, 8192)
CL_SPLIT = 2048  # entries of a row one wave walks (dppr_cluster_plan.hpp): a longer row is walked in pieces by k_cl_big
EPS = 1e-7


def graph_of(e, epoch=-1):
    row, col = e.read_out_graph(epoch)
    return e.V, row, col, len(col)


def orders_of(e, hd, k, min_p):
    return [e.topk(hd[1], k, min_p)[0]] if hd[0] == "slot" else [t[0] for t in e.group_topk(hd[1], k, min_p)]


def run(e, hd, k, min_p=0.0, min_size=1, epoch=-1, profile=True):
    """The call as a group call: (list of best, ids, cut_out, cut_in, vol), the arrays [n][k]."""
    if hd[0] == "group":
        return e.group_cluster(hd[1], k, min_p, min_size, epoch, profile)
    out = e.cluster(hd[1], k, min_p, min_size, epoch, profile)
    return ([out[0]],) + tuple(a[None, :] for a in out[1:]) if profile else [out]


def same_best(got, want, what):
    assert {k: v for k, v in got.items() if k != "best_phi"} == {k: v for k, v in want.items() if k != "best_phi"}, (what, got, want)
    assert bits(got["best_phi"]) == bits(want["best_phi"]), (what, got, want)


def check(e, hd, graph, k, min_p=0.0, min_size=1, epoch=-1, what=""):
    """One call with every array and one with none against the restatement; returns what the engine gave."""
    orders = orders_of(e, hd, k, min_p)
    got = run(e, hd, k, min_p, min_size, epoch)
    alone = run(e, hd, k, min_p, min_size, epoch, profile=False)
    assert len(got[0]) == len(alone) == len(orders)
    for i, order in enumerate(orders):
        tag = (what, hd, i, k, min_p, min_size)
        want = cluster_ref.cluster(*graph, order, k, min_size)
        assert want[0]["count"] == len(order) == min(k, len(order))
        same_best(got[0][i], want[0], tag)
        same_best(alone[i], want[0], tag + ("no arrays",))
        for g, w, name in zip(got[1:], want[1:], ("ids", "cut_out", "cut_in", "vol")):
            assert g.dtype == w.dtype and np.array_equal(g[i], w), tag + (name, g[i][:8], w[:8])
        L = len(order)
        assert np.all(got[1][i, L:] == -1) and all(np.all(a[i, L:] == 0) for a in got[2:]), tag
    return got


def rmat_window(directed):
    """R-MAT at scale 10, a window of 4000 edges with duplicates and a self loop; a slot and a 3-source group on the top sources."""
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    w1, w2 = e1[:4000].copy(), e2[:4000].copy()
    if not np.any(w1 == w2):
        w1, w2 = np.append(w1, w1[0]), np.append(w2, w1[0])
    assert len(np.unique(w1.astype(np.int64) * V + w2)) < len(w1) and np.any(w1 == w2)
    e = eng.Engine(V, len(w1), directed, 50)
    e.load_window(w1, w2)
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, 4000, directed, 16)]
    return e, srcs


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_equals_the_restatement(directed):
    e, srcs = rmat_window(directed)
    slot = e.add_source(srcs[0])
    gid = e.add_source_group(srcs[:3])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    graph = graph_of(e)
    assert max(len(o) for o in orders_of(e, ("group", gid), 8192, 0.0)) < 8192  # the largest k exceeds the qualifying count
    for hd in (("slot", slot), ("group", gid)):
        for k in KS:
            for min_p in (0.0, 1e-6):
                for min_size in (1, 5):
                    if min_size <= k:
                        check(e, hd, graph, k, min_p, min_size)
    got = run(e, ("group", gid), 1000)
    assert all(b["best_size"] > 0 and 0.0 <= b["best_phi"] < 1.0 for b in got[0])
    if directed:
        assert np.any(got[2] != got[3])
    e.close()


# 2, 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_a_prefix_does_not_depend_on_what_follows_and_a_symmetric_window_has_one_cut(directed):
    e, srcs = rmat_window(directed)
    gid = e.add_source_group(srcs[:3])
    e.group_init_solve(gid, EPS)
    short, long = run(e, ("group", gid), 64), run(e, ("group", gid), 1000)
    for a, b in zip(short[1:], long[1:]):
        assert np.array_equal(a, b[:, :64])
    assert all(b["count"] > 64 for b in long[0]) and np.all(long[2][:, :64] > 0)  # (the short order is a proper prefix of the long one)
    if not directed:
        for k in (64, 1000, 8192):
            got = run(e, ("group", gid), k)
            assert np.array_equal(got[2], got[3]), k
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_planted_partition_is_found():
    """Blocks of 40 and 60 vertices joined by three bridges (tests/test_cluster_plan.py holds the same for the exact fixed point):
    solved at 1e-9, far below the gap of 8e-4 in p across the boundary, the best prefix of sources 5, 0 and 39 is exactly block A."""
    V, und = planted_partition()
    e = eng.Engine(V, len(und), 0, 1)
    e.load_window(und[:, 0], und[:, 1])
    gid = e.add_source_group([5, 0, 39])
    slot = e.add_source(39)
    e.group_init_solve(gid, 1e-9)
    e.init_solve(slot, 1e-9)
    graph = graph_of(e)
    assert graph[3] == 2 * len(und)
    for hd in (("group", gid), ("slot", slot)):
        got = check(e, hd, graph, 100)
        for i, b in enumerate(got[0]):
            assert b == dict(count=100, best_size=40, best_cut=3, best_vol=489, best_phi=3.0 / 489.0), (hd, i, b)
            assert sorted(got[1][i, :40].tolist()) == list(range(40))
            den = np.minimum(got[4][i], graph[3] - got[4][i])
            phi = np.where(den > 0, got[2][i] / np.maximum(den, 1), np.inf)
            phi[39] = np.inf
            assert phi.min() >= 0.0207
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_group_width():
    e, srcs = rmat_window(1)
    graph = graph_of(e)
    for n in (1, 2, 5, 10, 16):
        gid = e.add_source_group(srcs[:n])
        e.group_init_solve(gid, EPS)
        for k in (65, 8192):
            got = check(e, ("group", gid), graph, k, what=f"n={n}")
            assert got[1].shape == (n, k)
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_rows_walked_in_pieces():
    """A star whose hub has CL_SPLIT + 300 leaves on an undirected window: its out-row and its in-row are both longer than one
    wave walks, so both go through the chunk list. A few hundred edges among the leaves, and a path hanging off leaf 1. Sources: the hub
    (position 0 of its order) and the end of the path (the hub deep in the prefix)."""
    text = open(os.path.join(ROOT, "dynamicppr_amd", "csrc", "dppr_cluster_plan.hpp")).read()
    assert int(re.search(r"constexpr int CL_SPLIT = (\d+);", text).group(1)) == CL_SPLIT
    leaves, path = CL_SPLIT + 300, 6
    rng = np.random.default_rng(17)
    a, b = rng.integers(1, leaves + 1, 400), rng.integers(1, leaves + 1, 400)
    chain = np.arange(leaves + 1, leaves + 1 + path)
    w1 = np.concatenate([np.zeros(leaves, dtype=np.int64), a, [1], chain[:-1]]).astype(np.int32)
    w2 = np.concatenate([np.arange(1, leaves + 1), b, [chain[0]], chain[1:]]).astype(np.int32)
    perm = rng.permutation(len(w1))
    V, far = 4096, int(chain[-1])
    e = eng.Engine(V, len(w1), 0, 1)
    e.load_window(w1[perm], w2[perm])
    graph = graph_of(e)
    deg = np.diff(graph[1])
    assert deg[0] > CL_SPLIT and np.sort(deg)[-2] < 64
    gid = e.add_source_group([0, far])
    slot = e.add_source(far)
    e.group_init_solve(gid, 1e-9)
    e.init_solve(slot, 1e-9)
    for k in (1, 5, 1000, 8192):
        got = check(e, ("group", gid), graph, k)
        check(e, ("slot", slot), graph, k)
        assert got[1][0, 0] == 0
        if k >= 1000:
            at = int(np.nonzero(got[1][1] == 0)[0][0])
            assert 3 <= at < 100, at
            assert got[2][1, at] - got[2][1, at - 1] > CL_SPLIT // 2  # the hub's row is what the cut grows by there
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_after_slides_renumberings_and_on_the_right_epoch_only():
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + (batches + 8) * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c, n_epochs=2)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    slot = e.add_source(0)
    gid = e.add_source_group([0, 1, 2])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    done, newest, renumbered = 0, 0, True
    while done < batches or renumbered:  # (a renumbering drops the older epoch: end on a slide that kept it)
        assert done < batches + 8 and not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        before = e.id_space()["renumberings"]
        newest = e.slide(*g.new_stream())
        e.update(slot, EPS)
        e.group_update(gid, EPS)
        renumbered = e.id_space()["renumberings"] > before
        done += 1
    sp = e.id_space()
    assert sp["parked"] > 0 and sp["renumberings"] > 0, sp
    graph = graph_of(e)
    in_window = np.zeros(V, dtype=bool)
    w1, w2 = g.window_edges()
    in_window[w1] = in_window[w2] = True
    for hd in (("slot", slot), ("group", gid)):
        for k in (100, 8192):
            got = check(e, hd, graph, k, what="after slides")
        for i in range(got[1].shape[0]):  # a parked vertex (no edge in the window, p > 0) inside the prefix: a row of degree 0
            ids = got[1][i][got[1][i] >= 0]
            at = np.nonzero(~in_window[ids])[0]
            assert len(at) and at[0] > 0 and got[4][i, at[0]] == got[4][i, at[0] - 1]
    # the states stand on the newest epoch: the older one is resident but refused, an evicted one is no epoch at all
    L, h = e._L, e._h
    best = (eng.Cluster * 3)()
    for b in best:
        b.count, b.best_phi = 7, 2.5
    ids = np.full(3 * 16, 7, dtype=np.int32)
    arrs = [np.full(3 * 16, 7, dtype=np.int64) for _ in range(3)]

    def rcs(epoch):
        a = (epoch, 16, 0.0, 1, C.addressof(best), ids.ctypes.data, *[x.ctypes.data for x in arrs])
        return L.dppr_cluster(h, slot, *a), L.dppr_group_cluster(h, gid, *a)

    def untouched():
        return all(b.count == 7 and b.best_phi == 2.5 for b in best) and np.all(ids == 7) and all(np.all(x == 7) for x in arrs)

    e.read_out_graph(newest - 1)  # (resident)
    assert rcs(newest - 1) == (-1, -1) and untouched()
    assert b"another epoch" in L.dppr_last_error(h)
    assert rcs(newest - 2) == (-1, -1) and rcs(newest + 1) == (-1, -1) and untouched()
    assert b"not resident" in L.dppr_last_error(h)
    assert rcs(newest) == (0, 0) and not untouched()
    # a state set by dppr_write stands on no epoch in particular: any resident one is accepted
    p, r = e.read(slot)
    e.write(slot, p, r)
    for epoch in (newest - 1, newest, -1):
        check(e, ("slot", slot), graph_of(e, epoch), 8192, epoch=epoch, what=f"written, epoch {epoch}")
    assert L.dppr_cluster(h, slot, newest - 2, 16, 0.0, 1, C.addressof(best), None, None, None, None) == -1
    e.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing():
    e, srcs = rmat_window(1)
    slot = e.add_source(srcs[0])
    gid = e.add_source_group(srcs[:2])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    L, h = e._L, e._h
    best = (eng.Cluster * 2)()
    ids = np.empty(2 * 8, dtype=np.int32)
    arrs = [np.empty(2 * 8, dtype=np.int64) for _ in range(3)]

    def fill():
        for b in best:
            b.count, b.best_size, b.best_cut, b.best_vol, b.best_phi = 7, 7, 7, 7, 2.5
        ids[:] = 7
        for x in arrs:
            x[:] = 7

    def untouched():
        return (all(b.as_dict() == dict(count=7, best_size=7, best_cut=7, best_vol=7, best_phi=2.5) for b in best) and np.all(ids == 7)
                and all(np.all(x == 7) for x in arrs))

    def rcs(slot_=None, gid_=None, epoch=-1, k=8, min_p=0.0, min_size=1, pbest=C.addressof(best)):
        a = (epoch, k, min_p, min_size, pbest, ids.ctypes.data, *[x.ctypes.data for x in arrs])
        return L.dppr_cluster(h, slot if slot_ is None else slot_, *a), L.dppr_group_cluster(h, gid if gid_ is None else gid_, *a)

    fill()
    assert rcs() == (0, 0) and not untouched()  # (the call as such is fine)
    fill()
    for k in (0, -1, eng.CLUSTER_MAX + 1, 2**31 - 1):
        assert rcs(k=k) == (-1, -1) and untouched(), k
    for min_p in (-1e-300, -1.0, float("nan"), float("-inf")):
        assert rcs(min_p=min_p) == (-1, -1) and untouched(), min_p
    for min_size in (0, -1, 9, 2**31 - 1):
        assert rcs(min_size=min_size) == (-1, -1) and untouched(), min_size
    assert rcs(pbest=None) == (-1, -1) and untouched()
    assert rcs(slot_=5, gid_=5) == (-1, -1) and rcs(slot_=-1, gid_=-1) == (-1, -1) and untouched()
    assert rcs(epoch=1) == (-1, -1) and rcs(epoch=7) == (-1, -1) and untouched()
    assert rcs(k=eng.CLUSTER_MAX, min_size=eng.CLUSTER_MAX, pbest=None) == (-1, -1) and untouched()
    # the limits themselves are fine (the arrays of this test hold 8 entries per source: none is passed)
    for k, ms in ((1, 1), (eng.CLUSTER_MAX, eng.CLUSTER_MAX), (eng.CLUSTER_MAX, 1)):
        assert L.dppr_cluster(h, slot, -1, k, 0.0, ms, C.addressof(best), None, None, None, None) == 0
        assert L.dppr_group_cluster(h, gid, 0, k, 0.0, ms, C.addressof(best), None, None, None, None) == 0
        if ms == eng.CLUSTER_MAX:  # (no order here is 8192 long: no prefix is eligible)
            assert all(0 < b.count < ms and b.best_size == 0 and b.best_cut == b.best_vol == 0 and b.best_phi == float("inf") for b in best)
    e.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_no_side_effects():
    """p and r read back bit-identical after the calls, the time of the last query is reported, and the next group_update gives
    the same bits as on an engine that never asked. The stream is a conflict-free one (tests/cf_stream.py): there the atomic sums of
    an update have no freedom in their order, so two engines that do the same give the same bits (on an R-MAT stream two plain
    engines already differ in the last bits of r), and a difference is the query's doing."""
    V, e1, e2, meta = conflict_free_stream(seed=1, **SMALL)
    W, c = SMALL["W"], SMALL["c"]
    sources = [int(x) for x in meta["sources"][:3]]
    states = []
    for ask in (True, False):
        g = orc.Graph(V, e1, e2, 1, W, c)
        e = eng.Engine(V, W, 1, c)
        e.load_window(*g.window_edges())
        gid = e.add_source_group(sources)
        slot = e.add_source(sources[0])
        e.group_init_solve(gid, CF_EPS)
        e.init_solve(slot, CF_EPS)
        reads = []
        for step in range(3):
            if ask:
                before = [e.group_read(gid, i) for i in range(3)] + [e.read(slot)]
                e.set_profiling(1)
                best = e.group_cluster(gid, 8192, profile=True)[0]
                assert e.query_ms() > 0 and all(b["count"] > 1 for b in best)
                e.cluster(slot, 1000, 1e-12, 2)
                assert e.query_ms() > 0
                e.set_profiling(0)
                after = [e.group_read(gid, i) for i in range(3)] + [e.read(slot)]
                for x, y in zip(before, after):
                    assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1]))
            assert not g.stream_updates()
            g.inc_construct(1)
            e.set_batch(*g.batch())
            e.slide(*g.new_stream())
            e.group_update(gid, CF_EPS)
            e.update(slot, CF_EPS)
            reads += [e.group_read(gid, i) for i in range(3)] + [e.read(slot)]
        states.append(reads)
        e.close()
    assert any(np.any(x[0] != y[0]) for x, y in zip(states[0][:4], states[0][4:8]))  # (the batches move the states)
    for x, y in zip(*states):
        assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1]))
