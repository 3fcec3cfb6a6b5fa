"""Every family of state queries beside the graph update of the NEXT batch (dppr_set_batch + dppr_slide_concurrent of batch k + 1 while
the states stand on epoch k): top-k and point reads, weighted top-k and score_at, changes, support and the sparse / dense exports, the
dense and sparse dot, walks and refine, cluster, subgraph, ranked top-k and rank_score_at. A graph update changes no solver state, so
-- in the caller's ids -- every result DURING and AFTER the slide of batch k + 1 is, bit for bit, the result of the same call made
before that slide started, also for a parked vertex the batch revives (its id changes, its rows move). On top of that the quiet
result is the numpy restatement each family's own test file uses (tests/*_ref.py and the `expected` helpers), over the dense reads
and the epoch's out-CSR by external id.

The rig is the one of tests/test_overlap_gpu.py (churn stream, W = 600, c = 60, two resident epochs, renumbering at 8 % / 8 parked),
with a slot, a 3- and a 10-source group and a 5-lane target group on ONE engine. The epoch of the last update is always named.

An exclusive slide that renumbers makes every older epoch unavailable (include/dppr.h, dppr_set_renumbering): after it the calls
that read the epoch's CSR (walks / refine, cluster, subgraph, the ranked specs with a degree factor or a neighbour exclusion) must
be REFUSED as "epoch not resident"; every other call must still give the quiet result.

Measured on an MI355X with this rig: a concurrent set_batch + slide takes 0.3 to 0.7 ms, a quiet pass of all ten families (about 85
calls) 10.4 ms, and a renumbering is due at one slide in three. So a slide is usually over before the first family called beside it
returns: which family overlaps is decided by the rotation (family k mod F first), and test 2 runs 120 batches (81 concurrent slides)
to give every family its share -- 6 (topk) to 18 (weighted) calls beside a slide per family, in both directions."""
import threading
import time

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests import cluster_ref, dot_ref, rank_ref, subgraph_ref
from tests.test_changes_gpu import expected as changes_expected
from tests.test_dot_gpu import put
from tests.test_export_gpu import Hip, want_sparse
from tests.test_overlap_gpu import staged_batches
from tests.test_renumbering_gpu import churn_stream
from tests.test_targets_gpu import lane_kinds
from tests.test_topk_gpu import expected as topk_expected
from tests.test_walks_gpu import device_rows, want_refine, want_walks
from tests.test_weighted_gpu import bits, expected as weighted_expected, fold

pytestmark = pytest.mark.gpu

V, N_STREAM, BAND, SEED = 4096, 9000, 400, 5
W, C, EPS = 600, 60, 1e-9
BATCHES = 40
BATCHES_BESIDE = 120     # test 2: a slide (~0.5 ms) is over before the first family called beside it returns, and one slide in three is
                         # exclusive (a renumbering is due): family k mod F came first beside 2 to 6 slides of 60 batches, 3 are asked for
K = 2048                 # above the largest support (1055, undirected): every vertex with p > 0 is returned
N_IDS, N_STARTS = 300, 64
WALKS, WALK_SEED = 64, 7
FAMILIES = ("topk", "point", "weighted", "changes", "export", "dot", "walks", "cluster", "subgraph", "ranked")
S, IN, OUT = eng.EXCLUDE_SEEDS, eng.EXCLUDE_IN_NEIGHBOURS, eng.EXCLUDE_OUT_NEIGHBOURS


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def eq(x, y):
    """Floating point by bit pattern (and the same type), everything else by value."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape:
        return False
    if x.dtype.kind == "f" or y.dtype.kind == "f":
        if x.dtype != y.dtype:
            return False
        return bool(np.array_equal(bits(x), bits(y))) if x.dtype == np.float64 else x.tobytes() == y.tobytes()
    return bool(np.array_equal(x, y))


def same(got, want, tag):
    """Two results of one family: dicts of lists of arrays."""
    assert got.keys() == want.keys(), (tag, sorted(map(str, got.keys() ^ want.keys())))
    for key in got:
        assert len(got[key]) == len(want[key]), (tag, key, len(got[key]), len(want[key]))
        for j, (a, b) in enumerate(zip(got[key], want[key])):
            assert eq(a, b), (tag, key, j, np.asarray(a).dtype, np.asarray(b).dtype, np.shape(a), np.shape(b),
                              np.asarray(a).ravel()[:6], np.asarray(b).ravel()[:6])


def refused(call):
    with pytest.raises(eng.DpprError, match="not resident"):
        call()


def flat_best(bests):
    return [np.array([b[name] for b in bests], dtype=np.int64) for name in ("count", "best_size", "best_cut", "best_vol")] + \
           [np.array([b["best_phi"] for b in bests], dtype=np.float64)]


class Rig:
    """The engine of the overlap test with its handles, the device buffers of the calls that need some, and the families."""

    def __init__(self, directed, hip, batches, full=True):
        self.directed, self.hip, self.batches = directed, hip, batches
        e1, e2 = churn_stream(V, N_STREAM, BAND, SEED)
        self.stage = staged_batches(V, e1, e2, directed, W, C, batches + 1)   # (one more: the vertices "the next batch names" of the last one)
        g = orc.Graph(V, e1, e2, directed, W, C)
        self.e = e = eng.Engine(V, W, directed, C, n_epochs=2)
        e.set_renumbering(1, growth_pct=8, min_parked=8)
        e.load_window(*g.window_edges())
        self.slot = e.add_source(0)
        self.g10 = e.add_source_group(list(range(10)))
        # handle -> (kind, id, lanes, the seeds of every lane)
        self.handles = {"slot": ("slot", self.slot, 1, [[0]]), "g10": ("group", self.g10, 10, [[i] for i in range(10)])}
        if full:
            self.g3 = e.add_source_group([0, 1, 2])
            kinds = lane_kinds(V, e1, np.random.default_rng(45))
            self.sets = [kinds[1], kinds[2]] + [(np.array([v], dtype=np.int32), np.array([1.0])) for v in (3, 4, 5)]
            self.tg = e.add_target_group(self.sets)
            self.handles["g3"] = ("group", self.g3, 3, [[0], [1], [2]])
            self.handles["tg"] = ("group", self.tg, 5, [s[0] for s in self.sets])
        e.init_solve(self.slot, EPS)
        for kind, hd, _, _ in self.handles.values():
            if kind == "group":
                e.group_init_solve(hd, EPS)
        self.small = "g3" if full else "g10"     # the group of the calls made on one narrow group
        self.wide = ["g10", "tg"] if full else ["g10"]
        self.marks = None
        rng = np.random.default_rng(77)
        self.weights = {h: (rng.standard_normal((16, self.handles[h][2])), rng.random((1, self.handles[h][2])) + 0.1) for h in self.wide}
        # device memory of the caller, obtained once (an allocation waits for the whole device)
        self.h64 = rng.standard_normal((3, V))
        self.h32 = self.h64.astype(np.float32)
        self.d_h64, self.d_h32_vm = put(hip, self.h64), put(hip, np.ascontiguousarray(self.h32.T))
        self.mask = (rng.random(V) < 0.5).astype(np.uint8)
        self.g32 = (rng.random(V) + 0.5).astype(np.float32)
        self.d_mask, self.d_g32 = put(hip, self.mask), put(hip, self.g32)
        self.d_dense = hip.alloc(8 * 10 * V)
        ns = self.handles[self.small][2]
        self.cap_sparse, self.cap_col = ns * V, ns * 2 * W
        self.d_ids, self.d_p, self.d_r = hip.alloc(4 * ns * max(V, K)), hip.alloc(8 * ns * max(V, K)), hip.alloc(8 * ns * V)
        self.d_rp, self.d_col = hip.alloc(8 * ns * (K + 1)), hip.alloc(4 * self.cap_col)
        self.sp_w = rng.random(5 * 40) + 0.1
        self.specs = {"null": None,
                      "deg, every exclusion": eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=S | IN | OUT),
                      "inv_deg, deny": eng.Engine.rank_spec(eng.FACTOR_INV_DEG, mask=eng.MASK_DENY, mask_dev=self.d_mask),
                      "dev f32, allow": eng.Engine.rank_spec(eng.FACTOR_DEV, self.d_g32, eng.F32, mask=eng.MASK_ALLOW, mask_dev=self.d_mask)}
        self.graph_specs = ("deg, every exclusion", "inv_deg, deny")   # (these read the epoch's CSR)

    # ---- the stream -------------------------------------------------------------------------------------------------------------
    def build(self, k, concurrent, box):
        """Batch k's graph update; box gets (epoch, start, end) or the exception."""
        try:
            t0 = time.perf_counter()
            self.e.set_batch(*self.stage[k - 1]["b"])
            ep = self.e.slide(*self.stage[k - 1]["n"], concurrent=concurrent)
            box.append((ep, t0, time.perf_counter()))
        except BaseException as err:  # (raised again by the thread that joins)
            box.append(err)

    def built(self, box):
        assert len(box) == 1
        if isinstance(box[0], BaseException):
            raise box[0]
        return box[0]

    def update(self, epoch):
        self.e.update(self.slot, EPS, epoch=epoch)
        for kind, hd, _, _ in self.handles.values():
            if kind == "group":
                self.e.group_update(hd, EPS, epoch=epoch)

    def dense(self):
        """handle -> ([p_i], [r_i]): the dense reads."""
        out = {}
        for h, (kind, hd, n, _) in self.handles.items():
            pr = [self.e.read(hd)] if kind == "slot" else [self.e.group_read(hd, i) for i in range(n)]
            out[h] = ([x[0] for x in pr], [x[1] for x in pr])
        return out

    def mark(self):
        for kind, hd, _, _ in self.handles.values():
            (self.e.mark if kind == "slot" else self.e.group_mark)(hd)
        self.marks = {h: ps for h, (ps, _) in self.dense().items()}

    def probe(self, k):
        """The ids of batch k's point queries: the vertices batch k + 1 names (the parked ones among them -- revived by it -- first),
        parked vertices, vertices never named and live ones, interleaved; the first N_STARTS are the starts of the walks."""
        m, sp = self.e.id_map(), self.e.id_space()
        parked = np.nonzero(m >= V - sp["parked"])[0]
        never = np.nonzero(m < 0)[0]
        live = np.nonzero((m >= 0) & (m < sp["ids"]))[0]
        nxt = np.unique(np.concatenate(self.stage[k]["n"]))
        revived = np.intersect1d(nxt, parked)
        rng = np.random.default_rng(1000 + k)
        lists = [rng.permutation(x) for x in (np.setdiff1d(nxt, revived), parked, never, live)]
        out, seen, i = [], set(), 0
        for v in revived[:16]:
            out.append(int(v))
            seen.add(int(v))
        while len(out) < N_IDS:
            for x in lists:
                if i < len(x) and int(x[i]) not in seen and len(out) < N_IDS:
                    out.append(int(x[i]))
                    seen.add(int(x[i]))
            i += 1
            assert i <= V
        ids = np.array(out, dtype=np.int32)
        assert len(np.unique(ids)) == N_IDS and len(never) > 0 and np.any(np.isin(ids, nxt)) and np.any(np.isin(ids, never))
        assert len(parked) == 0 or np.any(np.isin(ids, parked))
        self.ids, self.starts = ids, ids[:N_STARTS]
        self.sp_off = np.arange(6, dtype=np.int64) * 40
        self.sp_ids = np.concatenate([ids[j::5][:40] for j in range(5)]).astype(np.int32)   # 5 seed sets; every one holds vertices of the next batch
        return ids

    # ---- the families: call(name, epoch, resident) -> dict of lists of arrays ------------------------------------------------------
    def call(self, name, epoch, resident=True):
        return getattr(self, "q_" + name)(epoch, resident)

    def want(self, name, epoch, D):
        return getattr(self, "w_" + name)(epoch, D)

    def each(self):
        return self.handles.items()

    def q_topk(self, epoch, resident):
        e, out = self.e, {}
        for k in (10, K):
            for mp in (0.0, EPS):
                for h, (kind, hd, n, _) in self.each():
                    out[(h, k, mp)] = list(e.topk(hd, k, mp)) if kind == "slot" else [x for t in e.group_topk(hd, k, mp) for x in t]
        return out

    def w_topk(self, epoch, D):
        return {(h, k, mp): [x for p, r in zip(*D[h]) for x in topk_expected(p, r, k, mp)]
                for k in (10, K) for mp in (0.0, EPS) for h in self.handles}

    def q_point(self, epoch, resident):
        e = self.e
        return {h: list(e.read_at(hd, self.ids) if kind == "slot" else e.group_read_at(hd, self.ids)) for h, (kind, hd, n, _) in self.each()}

    def w_point(self, epoch, D):
        at = lambda cols, kind: cols[0][self.ids] if kind == "slot" else np.stack([c[self.ids] for c in cols], axis=1)
        return {h: [at(D[h][0], kind), at(D[h][1], kind)] for h, (kind, _, _, _) in self.each()}

    def q_weighted(self, epoch, resident):
        e, out = self.e, {}
        for h in self.wide:
            hd = self.handles[h][1]
            for j, w in enumerate(self.weights[h]):
                out[(h, "topk", j)] = [x for t in e.group_topk_weighted(hd, w, K) for x in t]
            out[(h, "score_at")] = [e.group_score_at(hd, self.weights[h][0], self.ids)]
        return out

    def w_weighted(self, epoch, D):
        out = {}
        for h in self.wide:
            cols = D[h][0]
            for j, w in enumerate(self.weights[h]):
                out[(h, "topk", j)] = [x for wj in w for x in weighted_expected(fold(cols, wj), K, 0.0)]
            out[(h, "score_at")] = [np.stack([fold(cols, wj)[self.ids] for wj in self.weights[h][0]], axis=1)]
        return out

    def q_changes(self, epoch, resident):
        e, out = self.e, {}
        for md in (0.0, 1e-12):
            for h, (kind, hd, n, _) in self.each():
                res = [e.changes(hd, 50, md, False)] if kind == "slot" else e.group_changes(hd, 50, md, False)
                out[(h, md)] = [np.asarray(x) for t in res for x in t]
        return out

    def w_changes(self, epoch, D):
        return {(h, md): [np.asarray(x) for now, was in zip(D[h][0], self.marks[h]) for x in changes_expected(now, was, 50, md)]
                for md in (0.0, 1e-12) for h in self.handles}

    DENSE_FORMS = ((eng.DENSE_P, eng.F64, eng.VERTEX_MAJOR), (eng.DENSE_P, eng.F32, eng.SOURCE_MAJOR), (eng.DENSE_R, eng.F64, eng.SOURCE_MAJOR),
                   (eng.DENSE_R, eng.F32, eng.VERTEX_MAJOR))

    def q_export(self, epoch, resident):
        e, hip, out = self.e, self.hip, {}
        out["support"] = [np.array([e.support(self.slot, 0.0)]), e.group_support(self.g10, EPS)]
        for mp in (0.0, EPS):
            out[("slot", mp)] = list(e.export_sparse(self.slot, mp, with_r=True))
            out[("g10", mp)] = list(e.group_export_sparse(self.g10, mp, with_r=True))
        hd = self.handles[self.small][1]
        off = e.group_export_sparse_dev(hd, 0.0, self.cap_sparse, self.d_ids, self.d_p, self.d_r)
        total = int(off[-1])
        out["sparse_dev"] = [off, hip.read(self.d_ids, 4 * total, np.int32), hip.read(self.d_p, 8 * total, np.float64),
                             hip.read(self.d_r, 8 * total, np.float64)]
        for which, dtype, layout in self.DENSE_FORMS:
            np_t = np.float32 if dtype == eng.F32 else np.float64
            if layout == eng.VERTEX_MAJOR:   # (a slot has the one layout)
                e.export_dense_dev(self.slot, self.d_dense, which, dtype)
                out[("slot dense", which, dtype)] = [hip.read(self.d_dense, np.dtype(np_t).itemsize * V, np_t)]
            e.group_export_dense_dev(self.g10, self.d_dense, which, dtype, layout)
            out[("g10 dense", which, dtype, layout)] = [hip.read(self.d_dense, np.dtype(np_t).itemsize * 10 * V, np_t)]
        return out

    def w_export(self, epoch, D):
        out = {}
        out["support"] = [np.array([np.count_nonzero(D["slot"][0][0] > 0.0)]), np.array([np.count_nonzero(p > EPS) for p in D["g10"][0]])]
        for mp in (0.0, EPS):
            out[("slot", mp)] = list(want_sparse(*D["slot"], mp))
            out[("g10", mp)] = list(want_sparse(*D["g10"], mp))
        out["sparse_dev"] = list(want_sparse(*D[self.small], 0.0))
        for which, dtype, layout in self.DENSE_FORMS:
            np_t = np.float32 if dtype == eng.F32 else np.float64
            if layout == eng.VERTEX_MAJOR:
                out[("slot dense", which, dtype)] = [D["slot"][which][0].astype(np_t)]
            cols = D["g10"][which]
            out[("g10 dense", which, dtype, layout)] = [np.ascontiguousarray(np.stack(cols, axis=0 if layout == eng.SOURCE_MAJOR else 1).astype(np_t)).reshape(-1)]
        return out

    def q_dot(self, epoch, resident):
        e, out = self.e, {}
        out["dense f64 fm"] = [e.group_dot_dense_dev(self.g10, self.d_h64, 3, eng.DENSE_P, eng.F64, eng.H_FEATURE_MAJOR)]
        out["dense f32 vm"] = [e.group_dot_dense_dev(self.g10, self.d_h32_vm, 3, eng.DENSE_P, eng.F32, eng.H_VERTEX_MAJOR)]
        for h in ("g10", self.small):
            out[("sparse", h)] = [e.group_dot_sparse(self.handles[h][1], self.sp_off, self.sp_ids, self.sp_w)]
        return out

    def w_dot(self, epoch, D):
        out = {"dense f64 fm": [dot_ref.dense(self.h64, D["g10"][0])], "dense f32 vm": [dot_ref.dense(self.h32.astype(np.float64), D["g10"][0])]}
        for h in ("g10", self.small):
            out[("sparse", h)] = [dot_ref.sparse(self.sp_off, self.sp_ids, self.sp_w, D[h][0])]
        return out

    def q_walks(self, epoch, resident):
        e = self.e
        calls = {"walks": lambda: [e.walks(self.starts, WALKS, WALK_SEED, epoch)]}
        for h in ("slot", "g10", self.small):
            kind, hd, _, _ = self.handles[h]
            calls[("refine", h)] = lambda kind=kind, hd=hd: list((e.refine_at if kind == "slot" else e.group_refine_at)(hd, self.starts, WALKS, WALK_SEED, epoch))
        return self.run_epoch_calls(calls, resident)

    def run_epoch_calls(self, calls, resident):
        """The calls of a family that name the epoch: their results -- or, once a renumbering has made the epoch unavailable, refused."""
        if resident:
            return {key: c() for key, c in calls.items()}
        for c in calls.values():
            refused(c)
        return {}

    def w_walks(self, epoch, D):
        rows = device_rows(self.e, epoch)
        ends = want_walks(rows, self.starts, WALKS, WALK_SEED)
        out = {"walks": [ends]}
        for h in ("slot", "g10", self.small):
            est, corr, sumsq = want_refine(ends, D[h][0], D[h][1], self.starts)
            out[("refine", h)] = [x[:, 0] for x in (est, corr, sumsq)] if h == "slot" else [est, corr, sumsq]
        return out

    def q_cluster(self, epoch, resident):
        e, calls = self.e, {}
        for h, (kind, hd, n, _) in self.each():
            if kind == "slot":
                def c(hd=hd):
                    best, ids, co, ci, vol = e.cluster(hd, K, epoch=epoch, profile=True)
                    return flat_best([best]) + [ids[None, :], co[None, :], ci[None, :], vol[None, :]]
            else:
                def c(hd=hd):
                    best, ids, co, ci, vol = e.group_cluster(hd, K, epoch=epoch, profile=True)
                    return flat_best(best) + [ids, co, ci, vol]
            calls[h] = c
        return self.run_epoch_calls(calls, resident)

    def orders(self, D, h):
        return [topk_expected(p, r, K, 0.0) for p, r in zip(*D[h])]

    def w_cluster(self, epoch, D):
        row, col = self.e.read_out_graph(epoch)
        out = {}
        for h in self.handles:
            lanes = [cluster_ref.cluster(V, row, col, len(col), o[0], K, 1) for o in self.orders(D, h)]
            out[h] = flat_best([l[0] for l in lanes]) + [np.stack([l[j] for l in lanes]) for j in (1, 2, 3, 4)]
        return out

    def q_subgraph(self, epoch, resident):
        e, hip, calls = self.e, self.hip, {}
        for h, (kind, hd, n, _) in self.each():
            if kind == "slot":
                def c(hd=hd):
                    cnt, ids, p, rp, col = e.subgraph(hd, K, 0.0, epoch)
                    return [np.array([cnt]), np.array([0, len(col)]), ids[None, :], p[None, :], rp[None, :], col]
            else:
                def c(hd=hd):
                    return list(e.group_subgraph(hd, K, 0.0, epoch))
            calls[h] = c

        def dev():
            hd, n = self.handles[self.small][1], self.handles[self.small][2]
            cnt, off = e.group_subgraph_dev(hd, K, 0.0, self.cap_col, self.d_ids, self.d_p, self.d_rp, self.d_col, epoch)
            total = int(off[-1])
            assert total <= self.cap_col
            return [cnt, off, hip.read(self.d_ids, 4 * n * K, np.int32).reshape(n, K), hip.read(self.d_p, 8 * n * K, np.float64).reshape(n, K),
                    hip.read(self.d_rp, 8 * n * (K + 1), np.int64).reshape(n, K + 1), hip.read(self.d_col, 4 * total, np.int32)]
        calls["dev"] = dev
        return self.run_epoch_calls(calls, resident)

    def w_subgraph(self, epoch, D):
        row, col = self.e.read_out_graph(epoch)
        out = {}
        for h in self.handles:
            tops = self.orders(D, h)
            cnt, off, ids, rp, cl = subgraph_ref.subgraph(V, row, col, [t[0] for t in tops], K)
            p = np.zeros((len(tops), K))
            for i, t in enumerate(tops):
                p[i, :len(t[1])] = t[1]
            out[h] = [cnt, off, ids, p, rp, cl]
        out["dev"] = out[self.small]
        return out

    def q_ranked(self, epoch, resident):
        e, out = self.e, {}
        for what, spec in self.specs.items():
            calls = {}
            for h in ["slot"] + self.wide:
                kind, hd, _, _ = self.handles[h]
                if kind == "slot":
                    calls[(what, h, "topk")] = lambda hd=hd, spec=spec: list(e.topk_ranked(hd, K, 0.0, spec, epoch))
                    calls[(what, h, "score_at")] = lambda hd=hd, spec=spec: [e.rank_score_at(hd, self.ids, spec, epoch)]
                else:
                    calls[(what, h, "topk")] = lambda hd=hd, spec=spec: [x for t in e.group_topk_ranked(hd, K, 0.0, spec, epoch) for x in t]
            hd = self.handles[self.wide[-1]][1]
            calls[(what, self.wide[-1], "score_at")] = lambda hd=hd, spec=spec: [e.group_rank_score_at(hd, self.ids, spec, epoch)]
            out.update(self.run_epoch_calls(calls, resident or what not in self.graph_specs))
        return out

    def w_ranked(self, epoch, D):
        row, col = self.e.read_out_graph(epoch)
        tails, heads = rank_ref.edges(row, col)
        deg = rank_ref.out_degree(V, tails)
        out = {}
        for what in self.specs:
            for h in ["slot"] + self.wide:
                cols = D[h][0]
                if what == "null":
                    sc = rank_ref.scores(cols)
                elif what == "deg, every exclusion":
                    sc = rank_ref.scores(cols, rank_ref.DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, self.handles[h][3], S | IN | OUT))
                elif what == "inv_deg, deny":
                    sc = rank_ref.scores(cols, rank_ref.INV_DEG, outdeg=deg, deny=self.mask)
                else:
                    sc = rank_ref.scores(cols, rank_ref.DEV, g=self.g32, allow=self.mask)
                out[(what, h, "topk")] = [x for s in sc for x in rank_ref.topk(s, K, 0.0)]
                if h == "slot":
                    out[(what, h, "score_at")] = [sc[0][self.ids]]
                elif h == self.wide[-1]:
                    out[(what, h, "score_at")] = [np.stack([s[self.ids] for s in sc], axis=1)]
        return out

    # ---- what the tests share ---------------------------------------------------------------------------------------------------
    def all_calls(self, epoch, resident=True):
        return {f: self.call(f, epoch, resident) for f in FAMILIES}

    def hold(self, got, want, tag, partial=False):
        """got == want for every family; partial: a family may lack the keys of its refused calls, never all of an epoch-free one."""
        for f in got:
            w = want[f] if not partial else {key: want[f][key] for key in got[f]}
            same(got[f], w, tag + (f,))

    def restate(self, R0, epoch, tag, families=FAMILIES):
        D = self.dense()
        for f in families:
            same(R0[f], self.want(f, epoch, D), tag + (f, "numpy"))

    def returned_ids(self, R0):
        """Every id of the group_topk / topk (k = K, min_p = 0) results of R0."""
        return np.unique(np.concatenate([a for h in self.handles for a in R0["topk"][(h, K, 0.0)][0::3]]))


EPOCH_FREE = ("topk", "point", "weighted", "changes", "export", "dot")


def after_exclusive(rig, epoch, R0, renumbered, tag):
    """The pass after an exclusive slide: the quiet results; where the slide renumbered, the epoch's CSR is gone and its readers are refused."""
    R1 = rig.all_calls(epoch, resident=not renumbered)
    rig.hold(R1, R0, tag, partial=renumbered)
    if renumbered:
        assert all(R1[f].keys() == R0[f].keys() for f in EPOCH_FREE), tag
        assert not R1["walks"] and not R1["cluster"] and not R1["subgraph"], tag
        assert {k[0] for k in R1["ranked"]} == {"null", "dev f32, allow"}, tag


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_queries_after_the_next_slide_equal_the_quiet_ones(hip, directed):
    """The order of calls of the host program: batch k + 1 is built, then epoch k is queried. No thread."""
    rig = Rig(directed, hip, BATCHES)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    concurrent = revived = seen_returned = restated = 0
    after_renumbering = False
    t_pass = t_slide = 0.0
    for k in range(1, BATCHES + 1):
        rig.update(epoch)
        if k == 2:
            rig.mark()
        if rig.marks is None:
            rig.mark()          # (batch 1: the changes calls need a mark; the one the test keeps is taken after batch 2)
        rig.probe(k)
        t0 = time.perf_counter()
        R0 = rig.all_calls(epoch)
        t_pass += time.perf_counter() - t0
        if k in (1, 20, BATCHES) or after_renumbering:
            rig.restate(R0, epoch, (directed, k))
            restated += 1
            after_renumbering = False
        if k == BATCHES:
            break
        m0, sp0 = e.id_map(), e.id_space()
        box = []
        if e.renumbering_due():
            rig.build(k + 1, False, box)
            renumbered = e.id_space()["renumberings"] > sp0["renumberings"]
            after_exclusive(rig, epoch, R0, renumbered, (directed, k, "after the exclusive slide"))
            after_renumbering = renumbered
        else:
            rig.build(k + 1, True, box)        # (on this thread)
            t_slide += rig.built(box)[2] - rig.built(box)[1]
            rig.hold(rig.all_calls(epoch), R0, (directed, k, "after the concurrent slide"))
            concurrent += 1
            revived += e.id_space()["revivals"] - sp0["revivals"]
            moved = np.nonzero((m0 >= 0) & (e.id_map() != m0))[0]    # vertices the slide revived: they had an id, and it changed
            seen_returned += int(np.count_nonzero(np.isin(moved, rig.returned_ids(R0))))
        epoch = rig.built(box)[0]
    sp = e.id_space()
    print(f"directed={directed}: {concurrent} concurrent slides ({1e3 * t_slide / max(concurrent, 1):.2f} ms each), a quiet pass of all families "
          f"{1e3 * t_pass / BATCHES:.1f} ms, revived by a concurrent slide {revived}, of them in a returned top-k order {seen_returned}, "
          f"restated at {restated} batches, {sp}")
    assert sp["renumberings"] >= 1 and revived >= 1 and seen_returned >= 1 and restated >= 4, (sp, revived, seen_returned, restated)
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_queries_beside_a_concurrent_slide(hip, directed):
    """Batch k + 1 is built on a builder thread while this thread calls the families round-robin, starting with family k mod F; a
    call counts as beside when its interval and the builder's set_batch + slide intersect."""
    rig = Rig(directed, hip, BATCHES_BESIDE)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    F = len(FAMILIES)
    beside = dict.fromkeys(FAMILIES, 0)
    revived_beside = slides = 0
    t_slide = 0.0
    for k in range(1, BATCHES_BESIDE):
        rig.update(epoch)
        if k <= 2:
            rig.mark()
        rig.probe(k)
        R0 = rig.all_calls(epoch)
        box = []
        if e.renumbering_due():
            before = e.id_space()["renumberings"]
            rig.build(k + 1, False, box)
            after_exclusive(rig, epoch, R0, e.id_space()["renumberings"] > before, (directed, k, "after the exclusive slide"))
        else:
            before = e.id_space()["revivals"]
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            calls, i = [], k
            th.start()
            try:
                while th.is_alive():
                    f = FAMILIES[i % F]
                    q0 = time.perf_counter()
                    got = rig.call(f, epoch)
                    calls.append((f, q0, time.perf_counter()))
                    same(got, R0[f], (directed, k, "beside", f))
                    i += 1
            finally:
                th.join()
            _, b0, b1 = rig.built(box)
            for f, q0, q1 in calls:
                beside[f] += 1 if q0 < b1 and q1 > b0 else 0
            rig.hold(rig.all_calls(epoch), R0, (directed, k, "after the join"))
            revived_beside += e.id_space()["revivals"] - before
            slides += 1
            t_slide += b1 - b0
        epoch = rig.built(box)[0]
    print(f"directed={directed}: calls beside a slide per family {beside}, {slides} concurrent slides of {1e3 * t_slide / max(slides, 1):.2f} ms, "
          f"revivals beside {revived_beside}, {e.id_space()}")
    assert min(beside.values()) >= 3 and revived_beside >= 1, (beside, revived_beside)
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
OVERLAPPED = {}


@pytest.mark.parametrize("family", FAMILIES)
def test_first_call_of_a_family_beside_a_slide(hip, family):
    """The first call ever of a family on an engine is where its workspaces are made (and a grown buffer released): here it is issued
    while the builder thread is alive. Whether it truly overlapped is summed up by the test below."""
    rig = Rig(1, hip, 8, full=False)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]
    k = 1
    while True:
        rig.update(epoch)
        if k == 2:
            rig.mark()
        if k >= 4 and not e.renumbering_due():
            break
        assert k < 8
        box = []
        rig.build(k + 1, not e.renumbering_due(), box)
        epoch = rig.built(box)[0]
        k += 1
    rig.probe(k)
    box = []
    th = threading.Thread(target=rig.build, args=(k + 1, True, box))
    th.start()
    try:
        q0 = time.perf_counter()
        first = rig.call(family, epoch)
        q1 = time.perf_counter()
    finally:
        th.join()
    _, b0, b1 = rig.built(box)
    OVERLAPPED[family] = q0 < b1 and q1 > b0
    same(rig.call(family, epoch), first, (family, "after the join"))
    rig.restate({family: first}, epoch, (family,), families=(family,))
    e.close()


def test_most_first_calls_overlapped_their_slide():
    assert set(OVERLAPPED) == set(FAMILIES), "runs after test_first_call_of_a_family_beside_a_slide of this module"
    print("first calls that overlapped the slide:", OVERLAPPED)
    assert 2 * sum(OVERLAPPED.values()) >= len(FAMILIES), OVERLAPPED


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_marks_follow_vertices_revived_beside(hip):
    """Marks are kept by external id, state rows by internal id: with no update in between, nothing has changed against a mark
    before, during and after a concurrent slide that revives a vertex with p > 0 (its rows move); after the next update the
    changes are those of p_now - p_marked by external id."""
    rig = Rig(1, hip, BATCHES)
    e = rig.e
    box = []
    rig.build(1, False, box)
    epoch = rig.built(box)[0]

    def nothing_moved(tag):
        for h, (kind, hd, n, _) in rig.each():
            res = [e.changes(hd, 50)] if kind == "slot" else e.group_changes(hd, 50)
            assert len(res) == n
            for ids, d, p, moved in res:
                assert len(ids) == 0 and len(d) == 0 and len(p) == 0 and moved == 0, (tag, h, ids[:8], d[:8], moved)

    found = checked = False
    for k in range(1, BATCHES):
        rig.update(epoch)
        if found:
            D = rig.dense()
            for md in (0.0, 1e-12):
                for h, (kind, hd, n, _) in rig.each():
                    res = [e.changes(hd, 50, md)] if kind == "slot" else e.group_changes(hd, 50, md)
                    for i in range(n):
                        want = changes_expected(D[h][0][i], rig.marks[h][i], 50, md)
                        assert all(eq(np.asarray(a), np.asarray(b)) for a, b in zip(res[i], want)), (k, h, i, md)
                    assert any(t[3] > 0 for t in res), (k, h, md)     # (the update moved something: the check is not vacuous)
            checked = True
            break
        rig.mark()
        nothing_moved((k, "before"))
        box = []
        if e.renumbering_due():
            rig.build(k + 1, False, box)
            nothing_moved((k, "after the exclusive slide"))
        else:
            m0, D = e.id_map(), rig.dense()
            th = threading.Thread(target=rig.build, args=(k + 1, True, box))
            th.start()
            try:
                while th.is_alive():
                    nothing_moved((k, "beside"))
            finally:
                th.join()
            nothing_moved((k, "after"))
            moved = np.nonzero((m0 >= 0) & (e.id_map() != m0))[0]
            found = any(np.any(p[moved] > 0) for ps, _ in D.values() for p in ps)
        epoch = rig.built(box)[0]
    assert found and checked, (found, checked, e.id_space())
    e.close()
