"""Conflict-free layered streams (tests/cf_stream.py) on the CPU: the stream keeps its two invariants in every window, the
oracle's frontiers are conflict-free on it, and on such streams the oracle's schedules agree bit for bit -- with each
other and with a short numpy restatement of schedule C.

These are the premises of tests/test_conflict_free_gpu.py, which holds every sweep and push form of the engine to the
oracle bit for bit on the same streams. Only directed streams are built: an undirected edge runs both ways, so no
vertex set can be "dead" (receive residual but never send it back) and no row is guaranteed a single term.

The reference's FAST_FRONTIER (1) and VANILLA (3) variants zero a frontier residual at the snapshot and have no repair
step; schedule C repairs with (r + t) - x. Those differ only where a frontier vertex receives a term in its own sweep,
which conflict-free streams exclude, so variants 1 and 3 equal schedule C bit for bit here too.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.cf_stream import conflict_free_stream

ALPHA = 0.15
EPS = 1e-9
SMALL = dict(V=1 << 14, levels=6, W=40000, c=2000, batches=6, fan_max=3000, dup_frac=0.05)


def small(seed, **kw):
    return conflict_free_stream(seed=seed, **dict(SMALL, **kw))


# ------------------------------------------------------------------ the numpy restatement of schedule C
def legal(r, phase, eps):
    return r > eps if phase == 0 else r < -eps


def np_loop(p, r, w1, w2, V, eps, phase, merged=False):
    """Schedule C (orc_sync_main_loop; merged=True: orc_merged_main_loop) for streams on which every row receives at most
    one term per sweep. Returns the frontiers. Snapshot x = r[F], p[F] += a x; one term (1 - a) x / (outdeg + 1) per row,
    added as r[v] + t; r[F] -= x; next frontier: threshold crossings and repaired vertices still legal (merged: every
    touched vertex with |r| > eps)."""
    deg1 = np.bincount(w1, minlength=V) + 1.0
    sel_ok = (lambda v: np.abs(v) > eps) if merged else (lambda v: legal(v, phase, eps))
    F = np.flatnonzero(sel_ok(r))
    out = []
    while F.size:
        out.append(F)
        x = np.zeros(V)
        x[F] = r[F]
        p[F] = p[F] + ALPHA * x[F]
        inF = np.zeros(V, bool)
        inF[F] = True
        sel = inF[w2]
        tails, heads = w1[sel], w2[sel]
        assert len(np.unique(tails)) == len(tails), "a row receives two terms in one sweep"
        t = (1.0 - ALPHA) * x[heads] / deg1[tails]
        prer = r[tails]
        cur = prer + t
        r[tails] = cur
        r[F] = r[F] - x[F]
        if merged:
            touched = np.union1d(tails, F)
            F = touched[np.abs(r[touched]) > eps]
        else:
            crossed = tails[~legal(prer, phase, eps) & legal(cur, phase, eps)]
            F = np.union1d(crossed, F[legal(r[F], phase, eps)])
    return out


def np_stream_update(p, r, b1, b2, ins, deg_after, source):
    """CopyOutDegree + RevertOutDegree, then IncrementalBatchUpdate in record order (orc_stream_update)."""
    predeg = {}
    for u, v in zip(b1.tolist(), b2.tolist()):
        predeg[u] = int(deg_after[u])
        predeg[v] = int(deg_after[v])
    for u, i in zip(b1.tolist(), ins.tolist()):
        predeg[u] += -1 if i else 1
    for u, v, i in zip(b1.tolist(), b2.tolist(), ins.tolist()):
        add = (1.0 - ALPHA) * float(p[v]) - float(p[u]) - ALPHA * float(r[u]) + ALPHA * (1.0 if u == source else 0.0)
        predeg[u] += 1 if i else -1
        q = add / (predeg[u] + 1) / ALPHA
        r[u] = float(r[u]) + q if i else float(r[u]) - q


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def drive(V, e1, e2, W, c, batches):
    """The oracle graph stepped batch by batch: yields (k, graph, window tails, window heads)."""
    g = orc.Graph(V, e1, e2, 1, W, c)
    yield 0, g, *g.window_edges()
    for k in range(1, batches + 1):
        assert not g.stream_updates()
        g.inc_construct(1)
        yield k, g, *g.window_edges()


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("churn", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_stream_invariants_and_shape(seed, churn):
    V, e1, e2, meta = small(seed, churn=churn)
    W, c, batches, level = SMALL["W"], SMALL["c"], SMALL["batches"], meta["level"]
    assert len(e1) == W + batches * c and not np.any(e1 == e2)
    lt, lh = level[e1], level[e2]
    assert not np.any((lt < 0) & (lh >= 0)), "an edge from D to L"
    spine = (lt >= 0) & (lh >= 0)
    assert np.all(lh[spine] == lt[spine] - 1) and np.array_equal(spine, meta["kind"] == 0)
    assert np.array_equal(meta["parent"][spine], e2[spine])
    for b in range(1, batches + 1):                   # invariant 2: one level parity among a batch's L tails
        rec = np.concatenate([np.arange((b - 1) * c, b * c), np.arange(W + (b - 1) * c, W + b * c)])
        par = np.unique(lt[rec][lt[rec] >= 0] % 2)
        assert len(par) == 1, b
    dens, big_in, big_out = set(), 0, 0
    for b in range(batches + 1):                      # invariant 1 in every window the engine sees
        w1, w2 = e1[b * c:b * c + W], e2[b * c:b * c + W]
        sp = spine[b * c:b * c + W]
        assert len(np.unique(w1[sp])) == sp.sum(), b
        big_in = max(big_in, np.bincount(w2[sp], minlength=V).max())
        deg = np.bincount(w1, minlength=V)
        big_out = max(big_out, deg.max())
        dens.update((deg[deg > 0] + 1).tolist())
        assert len(np.unique(np.stack([w1, w2]), axis=1)[0]) < W  # duplicate fan edges: a multigraph
    assert big_in >= 1000 and big_out >= 2048
    assert sum(1 for d in dens if d & (d - 1)) >= 50
    if churn:                                         # vertices leave: the first window's D vertices are mostly gone at the end
        first = np.unique(np.concatenate([e1[:W], e2[:W]]))
        last = np.unique(np.concatenate([e1[-W:], e2[-W:]]))
        assert len(np.setdiff1d(first, last)) > V // 20


def test_external_ids_are_permuted():
    V, e1, e2, meta = small(1)
    lev = meta["level"]
    assert not np.array_equal(np.flatnonzero(lev >= 0), np.arange((lev >= 0).sum()))
    assert np.all(lev[meta["sources"][:2]] == 0) and np.all(lev[meta["sources"][2:]] == 1)


@pytest.mark.parametrize("churn", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_frontiers_are_conflict_free(seed, churn):
    """On the oracle's traces of schedule C: no sweep holds a vertex together with its parent, no row receives two
    nonzero terms in one sweep; and the traces of schedule A hold the same sets."""
    V, e1, e2, meta = small(seed, churn=churn)
    W, c = SMALL["W"], SMALL["c"]
    src = int(meta["sources"][2])
    sc, sa = orc.State(V, src, EPS), orc.State(V, src, EPS)
    sweeps = 0
    for k, g, w1, w2 in drive(V, e1, e2, W, c, SMALL["batches"]):
        sc.trace(True)
        sa.trace(True)
        if k:
            sc.sync_inc_execute(g)
            sa.cilk_inc_execute(g)
        else:
            sc.sync_execute(g)
            sa.cilk_execute(g)
        parent = np.full(V, -1)
        sp = meta["level"][w2] >= 0
        parent[w1[sp]] = w2[sp]
        fc, fa = sc.traced_frontiers(), sa.traced_frontiers()
        assert len(fc) == len(fa) and len(fc) > 2
        for F, G in zip(fc, fa):
            assert np.array_equal(np.sort(F), np.sort(G))
            inF = np.zeros(V, bool)
            inF[F] = True
            assert not np.any(inF[parent[F][parent[F] >= 0]]), k
            rows = w1[inF[w2]]
            assert len(np.unique(rows)) == len(rows), k
        sweeps += len(fc)
    assert sweeps > 30


@pytest.mark.parametrize("churn", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_numpy_restatement_equals_schedule_c_and_a(seed, churn):
    """Schedule C (sync_execute / sync_inc_execute) equals the numpy restatement, and schedule A (cilk_execute /
    cilk_inc_execute) equals schedule C, bit for bit after every batch; the frontiers of the restatement are the oracle's."""
    V, e1, e2, meta = small(seed, churn=churn)
    W, c = SMALL["W"], SMALL["c"]
    for src in (int(meta["sources"][0]), int(meta["sources"][2])):
        sc, sa = orc.State(V, src, EPS), orc.State(V, src, EPS)
        p, r = np.zeros(V), np.zeros(V)
        for k, g, w1, w2 in drive(V, e1, e2, W, c, SMALL["batches"]):
            sc.trace(True)
            if k:
                sc.sync_inc_execute(g)
                sa.cilk_inc_execute(g)
                np_stream_update(p, r, *g.batch(), np.bincount(w1, minlength=V), src)
                fr = np_loop(p, r, w1, w2, V, EPS, 0) + np_loop(p, r, w1, w2, V, EPS, 1)
            else:
                sc.sync_execute(g)
                sa.cilk_execute(g)
                r[src] = 1.0
                fr = np_loop(p, r, w1, w2, V, EPS, 0)
            want = sc.traced_frontiers()
            assert len(fr) == len(want) and all(np.array_equal(a, np.sort(b)) for a, b in zip(fr, want)), k
            assert same(p, sc.p) and same(r, sc.r), (src, k)
            assert same(sa.p, sc.p) and same(sa.r, sc.r), (src, k)


@pytest.mark.parametrize("seed", [1, 2])
def test_merged_loop_equals_numpy_restatement(seed):
    V, e1, e2, meta = small(seed)
    W, c, div = SMALL["W"], SMALL["c"], 4
    src = int(meta["sources"][2])
    m = orc.State(V, src, EPS)
    p, r = np.zeros(V), np.zeros(V)
    for k, g, w1, w2 in drive(V, e1, e2, W, c, SMALL["batches"]):
        if k:
            m.merged_inc_execute(g, EPS / div)
            np_stream_update(p, r, *g.batch(), np.bincount(w1, minlength=V), src)
            np_loop(p, r, w1, w2, V, EPS / div, 0, merged=True)
        else:
            m.sync_execute(g)
            r[src] = 1.0
            np_loop(p, r, w1, w2, V, EPS, 0)
        assert same(p, m.p) and same(r, m.r), k


@pytest.mark.parametrize("variant", [1, 3])
def test_variants_equal_schedule_c(variant):
    V, e1, e2, meta = small(3)
    W, c = SMALL["W"], SMALL["c"]
    src = int(meta["sources"][2])
    sv, sc = orc.State(V, src, EPS), orc.State(V, src, EPS)
    for k, g, w1, w2 in drive(V, e1, e2, W, c, SMALL["batches"]):
        if k:
            sv.variant_inc_execute(g, variant)
            sc.sync_inc_execute(g)
        else:
            sv.variant_execute(g, variant)
            sc.sync_execute(g)
        assert same(sv.p, sc.p) and same(sv.r, sc.r), k
        assert sv.stats() == sc.stats()


def test_parents_in_frontier_streams_order_the_repair():
    """With invariant 2 dropped a vertex and its parent share frontiers (so the repair order (r + t) - x is visible), but every
    row still receives one term: the restatement still equals schedule C bit for bit, and schedule A does not."""
    V, e1, e2, meta = small(4, parents_in_frontier=True)
    W, c = SMALL["W"], SMALL["c"]
    src = int(meta["sources"][2])
    sc, sa = orc.State(V, src, EPS), orc.State(V, src, EPS)
    p, r = np.zeros(V), np.zeros(V)
    pairs, a_differs = 0, False
    for k, g, w1, w2 in drive(V, e1, e2, W, c, SMALL["batches"]):
        sc.trace(True)
        if k:
            sc.sync_inc_execute(g)
            sa.cilk_inc_execute(g)
            np_stream_update(p, r, *g.batch(), np.bincount(w1, minlength=V), src)
            np_loop(p, r, w1, w2, V, EPS, 0)
            np_loop(p, r, w1, w2, V, EPS, 1)
        else:
            sc.sync_execute(g)
            sa.cilk_execute(g)
            r[src] = 1.0
            np_loop(p, r, w1, w2, V, EPS, 0)
        assert same(p, sc.p) and same(r, sc.r), k
        a_differs |= not same(sa.r, sc.r)
        parent = np.full(V, -1)
        sp = meta["level"][w2] >= 0
        parent[w1[sp]] = w2[sp]
        for F in sc.traced_frontiers():
            inF = np.zeros(V, bool)
            inF[F] = True
            pairs += int(np.sum(inF[parent[F][parent[F] >= 0]]))
    assert pairs > 100 and a_differs
