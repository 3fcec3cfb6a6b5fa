"""The reference for weighted vertex sets as targets (dppr_add_target_group): numpy restatements over the raw window edges.

A lane with the seed vector h keeps p[u] + a r[u] == a h[u] + (1-a)/(outdeg(u)+1) * sum_{v in out(u)} p[v]; its exact value is the
fixed point of that relation with r = 0. src / dst are the DIRECTED edges of the window (tests.util.window_directed_edges)."""
import numpy as np

ALPHA = 0.15


def seed_vector(ids, weights, V):
    h = np.zeros(V)
    h[np.asarray(ids, dtype=np.int64)] = np.asarray(weights, dtype=np.float64)
    return h


def exact_p(h, src, dst, V, alpha=ALPHA, iters=600):
    """The fixed point of p = a h + (1-a)/(d+1) * (out-sum of p): `iters` Jacobi steps (a contraction by at most 1-a a step:
    0.85**600 < 1e-42). h is [V], or [V, n] for n lanes at once: one np.bincount per step over (edge, lane) pairs, every bin
    summed in edge order as the one-lane form sums it (the same bits)."""
    h = np.asarray(h, dtype=np.float64)
    scale = (1.0 - alpha) / (np.bincount(src, minlength=V) + 1.0)
    if h.ndim == 1:
        p = alpha * h
        for _ in range(iters):
            p = alpha * h + scale * np.bincount(src, weights=p[dst], minlength=V)
        return p
    n = h.shape[1]
    bins = (np.asarray(src, dtype=np.int64)[:, None] * n + np.arange(n)[None, :]).ravel()
    p = alpha * h
    for _ in range(iters):
        p = alpha * h + scale[:, None] * np.bincount(bins, weights=p[dst].ravel(), minlength=V * n).reshape(V, n)
    return p


def invariant_err(p, r, h, src, dst, V, alpha=ALPHA):
    """bench.py's invariant_max_err with a h for a [u == s]."""
    outdeg = np.bincount(src, minlength=V)
    acc = np.bincount(src, weights=p[dst], minlength=V)
    rhs = (1.0 - alpha) / (outdeg + 1.0) * acc + alpha * np.asarray(h, dtype=np.float64)
    return float(np.max(np.abs(p + alpha * r - rhs)))
