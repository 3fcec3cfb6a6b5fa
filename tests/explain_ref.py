"""The explain queries (dppr_explain_at / dppr_group_explain_at, include/dppr.h) in numpy, for the tests and for
tools/explain_times.py. The inputs are what the engine reports through its other calls: the dense columns of group_read (or read),
the out-CSR of the epoch by external id from read_out_graph, and the seeds of every lane. mult is np.unique over (tail, head), a
contribution is two `*` and one `/` per element (numpy rounds each to double, nothing fused), the contributor order is np.lexsort
over (head, -c) among c > 0, and a path is a plain Python loop."""
import numpy as np

ALPHA = 0.15
ONE_MINUS_ALPHA = 1.0 - 0.15   # 0x1.b333333333333p-1, the literal 0.85
END_SEED, END_DEPTH, END_DEAD, END_CYCLE = 0, 1, 2, 3


class Graph:
    """The distinct (tail, head) pairs of the stored edges with their multiplicities, grouped by tail."""

    def __init__(self, V, tails, heads):
        tails, heads = np.asarray(tails, dtype=np.int64), np.asarray(heads, dtype=np.int64)
        self.V = int(V)
        self.deg = np.bincount(tails, minlength=V).astype(np.int64)
        pair, mult = np.unique(tails * V + heads, return_counts=True)   # (one key per (tail, head): the pair, ordered by tail, then head)
        self.tail, self.head, self.mult = pair // V, pair % V, mult.astype(np.int64)
        self.start = np.searchsorted(self.tail, np.arange(V + 1))   # (np.unique sorts by tail, then head)
        self.distinct = np.diff(self.start).astype(np.int64)

    def row(self, u):
        lo, hi = self.start[u], self.start[u + 1]
        return self.head[lo:hi], self.mult[lo:hi]


def from_csr(row, col):
    row = np.asarray(row, dtype=np.int64)
    V = len(row) - 1
    return Graph(V, np.repeat(np.arange(V, dtype=np.int64), np.diff(row)), np.asarray(col, dtype=np.int64)[:row[-1]])


def seed_vector(V, seeds):
    """h of one lane: seeds is a vertex (a source lane), a list of (vertex, weight) pairs (a set lane) or None."""
    h = np.zeros(V)
    if seeds is None:
        return h
    if np.isscalar(seeds):
        h[int(seeds)] = 1.0
        return h
    for v, w in seeds:
        h[int(v)] = float(w)
    return h


def contributors(g, p, u):
    """(heads, mult, c) of vertex u in one lane, in the contributor order."""
    heads, mult = g.row(u)
    with np.errstate(all="ignore"):
        c = ((ONE_MINUS_ALPHA * p[heads]) * mult.astype(np.float64)) / np.float64(g.deg[u] + 1)
        keep = np.nonzero(c > 0)[0]   # (false for a NaN)
    keep = keep[np.lexsort((heads[keep], -c[keep]))]
    return heads[keep], mult[keep], c[keep]


def explain(g, cols, seeds, ids, f, depth):
    """The outputs of dppr_group_explain_at as a dict of arrays, vertex-major. cols: the dense p of every lane; seeds: one entry per
    lane for seed_vector."""
    ids = np.asarray(ids, dtype=np.int64)
    m, n = len(ids), len(cols)
    hs = [seed_vector(g.V, s) for s in seeds]
    out = {"deg": g.deg[ids].astype(np.int32), "distinct": g.distinct[ids].astype(np.int32),
           "self": np.zeros((m, n)), "nbr_count": np.zeros((m, n), np.int32), "nbr": np.full((m, n, f), -1, np.int32),
           "nbr_mult": np.zeros((m, n, f), np.int32), "nbr_c": np.zeros((m, n, f)),
           "len": np.zeros((m, n), np.int32), "end": np.zeros((m, n), np.int32), "path": np.full((m, n, depth + 1), -1, np.int32),
           "path_p": np.zeros((m, n, depth + 1)), "path_c": np.zeros((m, n, depth))}
    for i in range(n):
        p, h = np.asarray(cols[i], dtype=np.float64), hs[i]
        first = {}   # vertex -> (heads, mult, c) in contributor order

        def order(u):
            if u not in first:
                first[u] = contributors(g, p, u)
            return first[u]

        for j, v in enumerate(ids):
            v = int(v)
            out["self"][j, i] = ALPHA * h[v]
            heads, mult, c = order(v)
            k = min(f, len(heads))
            out["nbr_count"][j, i] = k
            out["nbr"][j, i, :k], out["nbr_mult"][j, i, :k], out["nbr_c"][j, i, :k] = heads[:k], mult[:k], c[:k]
            path, t, u = [v], 0, v
            while True:
                out["path"][j, i, t], out["path_p"][j, i, t] = u, p[u]
                if h[u] > 0:
                    end = END_SEED
                    break
                if t == depth:
                    end = END_DEPTH
                    break
                heads, mult, c = order(u)
                if len(heads) == 0:
                    end = END_DEAD
                    break
                if int(heads[0]) in path:
                    end = END_CYCLE
                    break
                out["path_c"][j, i, t] = c[0]
                u = int(heads[0])
                path.append(u)
                t += 1
            out["len"][j, i], out["end"][j, i] = t + 1, end
    return out


def slot_form(res):
    """The same dict as Engine.explain_at returns it for a one-lane call."""
    return {k: (v if v.ndim == 1 else v[:, 0].copy()) for k, v in res.items()}


def same(got, want, what=""):
    """Integers by array_equal, doubles by bit pattern; every key of `want`."""
    for k, w in want.items():
        a = got[k]
        assert a.shape == w.shape and a.dtype == w.dtype, (what, k, a.shape, w.shape, a.dtype, w.dtype)
        if w.dtype == np.float64:
            ok = np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(w).view(np.uint64))
        else:
            ok = np.array_equal(a, w)
        assert ok, (what, k, np.argwhere(a != w)[:4].tolist())
