"""The forward walks (dppr_walks) and the refined point queries (dppr_refine_at / dppr_group_refine_at) on the device against the
numpy restatement of tests/walk_ref.py over the rows the device holds (dppr_read_out_graph + dppr_debug_id_map): endpoints, est,
corr and sumsq are compared by bit pattern; the one tolerance in this file is Hoeffding's bound of the test that shows the gain."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import dot_ref, walk_ref
from tests.test_changes_gpu import Marked, bits
from tests.test_export_gpu import Hip, cols_of
from tests.test_renumbering_gpu import churn_stream
from tests.test_walk_plan import gain_scenario

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, (0xDEADBEEF << 32) | 5)
I32P = C.POINTER(C.c_int32)


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def device_rows(e, epoch=-1):
    """(row_ptr, col, ext2int, int2ext): the out-CSR of `epoch` by internal id, neighbours ascending, duplicates kept."""
    row, col = e.read_out_graph(epoch)
    x2i = e.id_map()
    rp, cl, i2e = walk_ref.internal_csr(e.V, row, col, x2i)
    return rp, cl, x2i.astype(np.int64), i2e


def want_walks(rows, starts, W, seed):
    return walk_ref.walks(rows[0], rows[1], rows[2], rows[3], starts, W, seed)


def want_refine(ends, ps, rs, ids):
    """est, corr, sumsq [m][n] from the dense reads and the endpoints [m][W], as include/dppr.h states them."""
    t = walk_ref.terms(ends, rs)  # [n][m][W]
    W = ends.shape[1]
    corr = dot_ref.fold(t) / float(W)
    est = np.stack(ps, axis=0)[:, np.asarray(ids, dtype=np.int64)] + corr
    return est.T, corr.T, dot_ref.fold(t * t).T


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), (what, got.ravel()[:4], want.ravel()[:4])


def refine(e, hd, ids, W, seed, epoch=-1, **kw):
    fn = e.refine_at if hd[0] == "slot" else e.group_refine_at
    out = fn(hd[1], ids, W, seed, epoch, **kw)
    return tuple(None if o is None else np.asarray(o).reshape(len(ids), -1) for o in out)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_endpoints_equal_the_restatement(hip, directed):
    """An R-MAT window at scale 10 with duplicate edges. Starts: the largest hub, a vertex with in-edges and out-degree 0 (directed),
    a vertex the stream never named, duplicates. W in {1, 63, 64, 65, 1000} x m in {1, 3, 130} x three seeds: a walk is a function of
    (start, number, seed), so ONE restatement per seed (m = 130, W = 1000) holds every smaller call as a slice."""
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    Wn, c = 4000, 50
    w1, w2 = e1[:Wn].astype(np.int64), e2[:Wn].astype(np.int64)
    assert len(np.unique(w1 * V + w2)) < Wn  # duplicate edges
    e = eng.Engine(V, Wn, directed, c)
    e.load_window(e1[:Wn], e2[:Wn])
    e.add_source_group([int(x) for x in datagen.top_sources(V, e1, e2, Wn, directed, 3)])
    rows = device_rows(e)
    row_ext, _ = e.read_out_graph()
    outdeg = np.diff(row_ext)
    hub = int(np.argmax(outdeg))
    unnamed = int(np.nonzero(rows[2] < 0)[0][0])
    special = [hub, unnamed, hub]
    if directed:
        sinks = np.nonzero((outdeg == 0) & (np.bincount(w2, minlength=V) > 0))[0]
        assert len(sinks)
        special[2] = int(sinks[0])
    rng = np.random.default_rng(31)
    starts = np.concatenate([special, [hub], rng.integers(0, V, 126)]).astype(np.int32)
    assert len(starts) == 130 and len(np.unique(starts)) < 130
    for seed in SEEDS:
        want = want_walks(rows, starts, 1000, seed)
        assert np.any(want < 0) and np.any(want >= 0) and np.all(want[1][want[1] >= 0] == unnamed)
        for m in (1, 3, 130):
            for W in (1, 63, 64, 65, 1000):
                got = e.walks(starts[:m], W, seed)
                assert np.array_equal(got, want[:m, :W]), (seed, m, W)
        for m, W in ((3, 65), (130, 1000)):
            d_out = hip.alloc(4 * m * W + 16)
            e.walks_dev(starts[:m], W, seed, d_out)
            raw = hip.read(d_out, 4 * m * W + 16)
            assert np.all(raw[4 * m * W:] == 0xAB)
            assert np.array_equal(raw[:4 * m * W].view(np.int32).reshape(m, W), want[:m, :W]), (seed, m, W, "device")
        hip.free_all()
    # one walk per thread: the same array
    e.set_walk_form(eng.WALK_PER_THREAD)
    for m, W in ((3, 65), (130, 1000)):
        assert np.array_equal(e.walks(starts[:m], W, SEEDS[2]), want[:m, :W]), ("per thread", m, W)
    e.set_walk_form(eng.WALK_REFILL)
    # another position in the call, the same walks
    assert np.array_equal(e.walks(starts[::-1].copy(), 65, SEEDS[2]), want[::-1, :65])
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_chain_does_not_depend_on_the_numbering():
    """Out-degree <= 1: the choice is the neighbour or death, so the endpoints are a function of the external graph alone. The
    edges enter the stream in a shuffled order, so internal ids are not the chain's order."""
    V, L, W, seed = 64, 40, 300, SEEDS[2]
    order = np.random.default_rng(8).permutation(L)
    e = eng.Engine(V, L, 1, 1)
    e.load_window(order.astype(np.int32), (order + 1).astype(np.int32))
    assert not np.array_equal(e.id_map()[:L + 1], np.arange(L + 1))
    starts = np.arange(V, dtype=np.int32)
    got = e.walks(starts, W, seed)
    # the loop: all walks at once, one step a pass
    v, w = np.repeat(np.arange(V), W), np.tile(np.arange(W), V)
    u, ends, alive = v.copy(), np.full(V * W, -1), np.ones(V * W, dtype=bool)
    for t in range(256):
        x0, x1, x2, _ = walk_ref.philox(w, v, t, 0, seed & 0xFFFFFFFF, seed >> 32)
        stop = alive & (x0 < walk_ref.STOP_BELOW)
        ends[stop] = u[stop]
        d = (u < L).astype(np.int64)  # vertex u has the edge u -> u + 1, or none
        alive &= ~stop & (walk_ref.pick(x1, x2, d).astype(np.int64) < d)
        u[alive] += 1
    assert np.array_equal(got, ends.reshape(V, W)) and np.any(got >= 0) and np.any(got < 0)
    assert np.all((got[L:] == -1) | (got[L:] == np.arange(L, V)[:, None]))  # no out-edge: itself or death
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_refine_equals_the_fold_of_the_dense_reads():
    """Slot and group widths 1, 2, 10, 16, before and after a batch; W = 65537 for one query (across a fold block); a vertex
    without a row; NULL out_corr / out_sumsq."""
    s = Marked(1, widths=(1, 2, 10, 16))
    seed = SEEDS[2]
    for batches in (0, 1):
        s.update(batches)
        x2i = s.e.id_map()
        norow = int(np.nonzero(x2i < 0)[0][0])
        ids = np.array([s.srcs[0], norow, s.srcs[1], int(np.nonzero(x2i >= 0)[0][-1]), s.srcs[0]], dtype=np.int32)
        ends = s.e.walks(ids, 1000, seed)
        assert np.array_equal(ends, want_walks(device_rows(s.e), ids, 1000, seed))
        long = s.e.walks(ids[:1], 65537, seed)
        for hd, n in s.handles():
            ps, rs = cols_of(s.e, hd, n)
            got = refine(s.e, hd, ids, 1000, seed)
            want = want_refine(ends, ps, rs, ids)
            for g, w, name in zip(got, want, ("est", "corr", "sumsq")):
                same(g, w, (batches, hd, n, name))
            assert np.any(got[1] != 0.0) and np.all(got[2] >= 0.0)
            est_only = refine(s.e, hd, ids, 1000, seed, corr=False, sumsq=False)
            assert est_only[1] is None and est_only[2] is None
            same(est_only[0], want[0], (batches, hd, n, "est alone"))
            got = refine(s.e, hd, ids[:1], 65537, seed)
            for g, w, name in zip(got, want_refine(long, ps, rs, ids[:1]), ("est", "corr", "sumsq")):
                same(g, w, (batches, hd, n, name, 65537))
    s.e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_it_is_worth_having():
    """Solve at eps = 1e-3, W = 2^16 walks, a fixed seed: for every queried vertex and source
        |est - pi^| <= R sqrt(2 ln(2 / delta) / W) + 1e-8 R,    R = max|r_i| read from the engine, delta = 1e-12,
    pi^ from the oracle's power iteration -- Hoeffding's bound for terms in [-R, R] plus the bias budget of include/dppr.h -- and
    plain p misses that bound at one queried vertex at least (tests/test_walk_plan.py holds both halves for the restatement)."""
    sc = gain_scenario()
    V, Wk = sc["V"], sc["walks"]
    g = orc.Graph(V, sc["e1"], sc["e2"], sc["directed"], sc["W"], sc["c"])
    e = eng.Engine(V, sc["W"], sc["directed"], sc["c"], schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    gid = e.add_source_group(sc["sources"])
    slot = e.add_source(sc["sources"][1])
    e.group_init_solve(gid, sc["eps"])
    e.init_solve(slot, sc["eps"])
    q = np.array(sc["queried"], dtype=np.int32)
    est, corr, sumsq = e.group_refine_at(gid, q, Wk, sc["seed"])
    est1, _, _ = e.refine_at(slot, q, Wk, sc["seed"])
    missed = 0
    for i, src in enumerate(sc["sources"]):
        p, r = e.group_read(gid, i)
        pi, _ = orc.pow_rev(g, src)
        R = float(np.max(np.abs(r)))
        bound = walk_ref.hoeffding(R, Wk)
        err, plain = np.abs(est[:, i] - pi[q]), np.abs(p[q] - pi[q])
        print(f"source {src}: R {R:.3e} bound {bound:.3e} refined {err} plain {plain}")
        assert 0 < R <= sc["eps"]
        assert np.all(err <= bound), (src, err, bound)
        missed += int(np.sum(plain > bound))
        # the standard error the caller derives is of the size of the error it stands for
        se = np.sqrt((sumsq[:, i] / Wk - corr[:, i] ** 2) / (Wk - 1))
        assert np.all(se < bound) and np.all(se > 0)
    assert missed >= 1
    p1, r1 = e.read(slot)
    pi1, _ = orc.pow_rev(g, sc["sources"][1])
    assert np.all(np.abs(est1 - pi1[q]) <= walk_ref.hoeffding(float(np.max(np.abs(r1))), Wk))
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_after_the_stream_moves_and_after_a_renumbering():
    V, W, c, eps, batches = 4096, 1500, 100, 1e-6, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 6)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    gid = e.add_source_group([0, 1, 2])
    e.group_init_solve(gid, eps)
    seed, checked_after = SEEDS[1], 0
    rng = np.random.default_rng(12)
    for k in range(1, batches + 1):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        before = e.id_space()["renumberings"]
        e.slide(*g.new_stream())
        e.group_update(gid, eps)
        sp = e.id_space()
        renumbered = sp["renumberings"] > before
        if k == 1 or renumbered or k == batches:
            rows = device_rows(e)
            parked = np.nonzero(rows[2] >= V - sp["parked"])[0] if sp["parked"] else np.zeros(0, dtype=np.int64)
            starts = np.concatenate([[0, int(e1[W + k * c - 1])], parked[:2], rng.integers(0, V, 60)]).astype(np.int32)
            ends = e.walks(starts, 130, seed)
            assert np.array_equal(ends, want_walks(rows, starts, 130, seed)), (k, renumbered)
            for j in range(len(parked[:2])):  # a parked vertex has no row in the graph: it stops at itself or dies
                assert np.all((ends[2 + j] == -1) | (ends[2 + j] == parked[j]))
            ps, rs = cols_of(e, ("group", gid), 3)
            for got, want, name in zip(refine(e, ("group", gid), starts, 130, seed), want_refine(ends, ps, rs, starts), ("est", "corr", "sumsq")):
                same(got, want, (k, name))
            checked_after += int(renumbered and len(parked) > 0)
    assert e.id_space()["renumberings"] >= 1 and checked_after >= 1
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(hip):
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    W, c, eps = 600, 20, 1e-6
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c, n_epochs=2)
    e.load_window(*g.window_edges())
    slot = e.add_source(int(e1[0]))
    gid = e.add_source_group([int(e1[0]), int(e2[0])])
    e.init_solve(slot, eps)
    e.group_init_solve(gid, eps)
    L, h = e._L, e._h
    ids = np.array([1, 2, 3], dtype=np.int32)
    ends = np.full(64, 7, dtype=np.int32)
    outs = [np.full(16, 2.5) for _ in range(3)]
    pid, pends = ids.ctypes.data_as(I32P), ends.ctypes.data

    def untouched():
        return np.all(ends == 7) and all(np.all(o == 2.5) for o in outs) and np.array_equal(ids, [1, 2, 3])

    def walks_rc(epoch=-1, starts=pid, m=3, W=4, dest=eng.DEST_HOST, out=pends):
        return L.dppr_walks(h, epoch, starts, m, W, 0, dest, out)

    def refine_rcs(epoch=-1, idp=pid, m=3, W=4, est=outs[0].ctypes.data):
        a = (idp, m, W, 0, est, outs[1].ctypes.data, outs[2].ctypes.data)
        return L.dppr_refine_at(h, slot, epoch, *a), L.dppr_group_refine_at(h, gid, epoch, *a)

    assert walks_rc() == 0 and not np.all(ends[:12] == 7) and np.all(ends[12:] == 7)  # (the call as such is fine)
    ends[:] = 7
    assert refine_rcs() == (0, 0)
    for o in outs:
        o[:] = 2.5
    # every limit
    for m, Wk in ((0, 4), (-1, 4), (eng.WALK_MAX_M + 1, 1), (3, 0), (3, -1), (1, eng.WALK_MAX_W + 1), (65, eng.WALK_MAX_W), (4096, 16385)):
        assert walks_rc(m=m, W=Wk) == -1 and refine_rcs(m=m, W=Wk) == (-1, -1) and untouched(), (m, Wk)
    # NULL pointers, a bad dest
    assert walks_rc(starts=None) == -1 and walks_rc(out=None) == -1 and walks_rc(dest=2) == -1 and walks_rc(dest=-1) == -1
    assert refine_rcs(idp=None) == (-1, -1) and refine_rcs(est=None) == (-1, -1) and untouched()
    # an id outside [0, V)
    for bad in (V, -1, 2**31 - 1):
        ids[1] = bad
        assert walks_rc() == -1 and refine_rcs() == (-1, -1) and np.all(ends == 7) and all(np.all(o == 2.5) for o in outs), bad
        ids[1] = 2
    # a host pointer passed as device memory; device memory that is too short or misaligned
    assert walks_rc(dest=eng.DEST_DEVICE) == -1 and untouched()
    d_small = hip.alloc(4 * 12)
    assert walks_rc(dest=eng.DEST_DEVICE, out=d_small) == 0
    assert walks_rc(dest=eng.DEST_DEVICE, out=d_small, W=5) == -1 and walks_rc(dest=eng.DEST_DEVICE, out=d_small + 2, W=1) == -1
    # a bad slot / group / epoch
    a = (pid, 3, 4, 0, outs[0].ctypes.data, None, None)
    assert L.dppr_refine_at(h, 5, -1, *a) == -1 and L.dppr_group_refine_at(h, 5, -1, *a) == -1 and L.dppr_refine_at(h, -1, -1, *a) == -1
    assert walks_rc(epoch=3) == -1 and refine_rcs(epoch=3) == (-1, -1) and untouched()
    # the stream moves by one batch, the states stay on epoch 0: walks run on either epoch, a refinement only on the state's
    assert not g.stream_updates()
    g.inc_construct(1)
    e.set_batch(*g.batch())
    assert e.slide(*g.new_stream()) == 1
    assert walks_rc(epoch=0) == 0 and walks_rc(epoch=1) == 0 and walks_rc(epoch=-1) == 0
    ends[:] = 7
    assert refine_rcs(epoch=1) == (-1, -1) and refine_rcs(epoch=-1) == (-1, -1) and untouched()
    assert b"biased" in L.dppr_last_error(h)
    assert refine_rcs(epoch=0) == (0, 0)
    for o in outs:
        o[:] = 2.5
    # an unconverged state
    e.incremental_batch_update(slot, 1)
    assert L.dppr_refine_at(h, slot, 1, pid, 3, 4, 0, outs[0].ctypes.data, None, None) == -1 and untouched()
    assert b"converged" in L.dppr_last_error(h)
    e.execute_main_loop(slot, 0, eps, 1)
    e.execute_main_loop(slot, 1, eps, 1)
    e.group_update(gid, eps, 1)
    assert refine_rcs(epoch=1) == (0, 0)
    for o in outs:
        o[:] = 2.5
    # an evicted epoch
    assert not g.stream_updates()
    g.inc_construct(1)
    e.set_batch(*g.batch())
    assert e.slide(*g.new_stream()) == 2
    assert walks_rc(epoch=0) == -1 and refine_rcs(epoch=0) == (-1, -1) and untouched()
    assert walks_rc(epoch=1) == 0 and refine_rcs(epoch=1) == (0, 0)
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_bystanders_and_ownership(hip):
    gc.collect()
    base = eng.live_bytes()
    s = Marked(0, widths=(2, 9))
    s.update(1)
    before = {hd: cols_of(s.e, hd, n) for hd, n in s.handles()}
    ids = np.arange(0, s.V, 7, dtype=np.int32)
    s.e.set_profiling(1)
    s.e.walks(ids, 257, 3)
    assert s.e.query_ms() > 0
    d_out = hip.alloc(4 * len(ids) * 64)
    s.e.walks_dev(ids, 64, 3, d_out)
    for hd, n in s.handles():
        refine(s.e, hd, ids, 257, 3)
        assert s.e.query_ms() > 0
    assert eng.live_bytes()[0] > base[0]
    for hd, n in s.handles():
        after = cols_of(s.e, hd, n)
        for x, y in zip(before[hd][0] + before[hd][1], after[0] + after[1]):
            assert np.array_equal(bits(x), bits(y)), hd
    s.e.close()
    hip.free_all()
    del s
    gc.collect()
    assert eng.live_bytes() == base
