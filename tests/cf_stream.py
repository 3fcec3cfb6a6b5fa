"""Conflict-free layered streams: directed sliding-window streams on which every sweep and push form has ONE order of
IEEE operations per residual, so p / r can be held to the oracle bit for bit ("Bars").

The vertices are split into a live set L, with levels 0 .. H-1, and a dead set D. Every stream edge is one of three kinds:

  * spine: a level-h vertex -> a level-(h-1) vertex (its "parent"). Heads are Zipf-distributed: long in-rows;
  * fan:   L -> D. Tails are Zipf-distributed: long out-rows, hub targets of the push forms, den = outdeg + 1 of every
           size. A fraction of them repeats the previous fan edge (the window is a multigraph);
  * dead:  D -> D. Rows that are scanned but only ever gather x = 0.

No edge runs from D to L and there are no self-loops. Two invariants hold in every window:

  1. at most one spine out-edge per L vertex: the spine edge of a tail comes back exactly W positions later (with a
     freshly drawn parent), so two spine edges of one tail are never in one window;
  2. the L tails of the positions [k c, (k + 1) c) all have the level parity k % 2. Batch b deletes chunk b - 1 and
     inserts chunk W / c + b - 1, and W / c is even: all L tails of a batch share one parity.

D never holds residual (it only reaches D), so an L row receives at most one nonzero term per sweep, from its parent;
and by induction over the sweeps no vertex is in a frontier together with its parent (sweep 0 is a subset of the batch
tails). tests/test_conflict_free_streams.py checks both on the oracle's traces.

`parents_in_frontier=True` drops invariant 2 (tails of both parities in every batch): a row still receives one
term, but a vertex and its parent can share a frontier, so the repair order (r + t) - x matters. Only the gather forms,
which fix that order, are held to the oracle on such streams.
"""
import numpy as np


def _zipf_cdf(n, s):
    w = 1.0 / np.arange(1, n + 1, dtype=np.float64) ** s
    c = np.cumsum(w)
    return c / c[-1]


def _zipf_for_top_share(n, share):
    """Exponent s of a Zipf law over n ranks whose top rank has probability `share` (bisection)."""
    lo, hi = 0.0, 8.0
    for _ in range(60):
        s = 0.5 * (lo + hi)
        top = 1.0 / np.sum(1.0 / np.arange(1, n + 1, dtype=np.float64) ** s)
        lo, hi = (s, hi) if top < share else (lo, s)
    return 0.5 * (lo + hi)


def _draw(rng, cdf, n):
    return np.minimum(np.searchsorted(cdf, rng.random(n), side="right"), len(cdf) - 1)


def level_sizes(n_live, levels):
    """Roots (level 0), a thin level 1 of hubs, then equal levels."""
    n0 = max(2, n_live // 4096)
    n1 = max(16, n_live // 128)
    rest = n_live - n0 - n1
    assert levels >= 3 and rest >= levels - 2
    out = [n0, n1] + [rest // (levels - 2)] * (levels - 2)
    out[-1] += rest - sum(out[2:])
    return out


def conflict_free_stream(V, levels, W, c, batches, seed, fan_max, dup_frac, churn=False, live_frac=0.6,
                         spine_s=1.6, dead_frac=0.16, parents_in_frontier=False):
    """(V, e1, e2, meta) of a stream of W + batches * c directed edges (external ids: a random permutation).

    meta: level[v] for every external id (-1 for D), parent[v] of every spine edge position (-1 elsewhere) and
    kind[pos] (0 spine, 1 fan, 2 dead) per stream position, and `sources`: the roots, then level-1 vertices with the
    largest subtrees in the initial window."""
    assert W % c == 0 and (W // c) % 2 == 0, "W / c must be an even integer (invariant 2)"
    rng = np.random.default_rng(seed)
    n = W + batches * c
    n_live = int(V * live_frac)
    n_dead = V - n_live
    sizes = level_sizes(n_live, levels)
    lev_int = np.concatenate([np.full(s, h, np.int32) for h, s in enumerate(sizes)] + [np.full(n_dead, -1, np.int32)])
    start = np.concatenate([[0], np.cumsum(sizes)])
    dead0 = n_live
    chunks = W // c
    chunk_par = (np.arange(n) // c) % 2                       # level parity of the L tails at each position

    # ---- the initial window's layout: every non-root L vertex gets one spine position in a chunk of its parity
    kind = np.where(rng.random(W) < dead_frac, 2, 1).astype(np.int8)
    tail = np.zeros(W, np.int64)
    nonroot = np.arange(start[1], n_live)
    if parents_in_frontier:
        groups = [(nonroot, np.arange(chunks))]
    else:
        groups = [(nonroot[lev_int[nonroot] % 2 == par], np.arange(par, chunks, 2)) for par in (0, 1)]
    for ids, mine in groups:
        ids = rng.permutation(ids)
        for k, piece in zip(mine, np.array_split(ids, len(mine))):
            assert 2 * len(piece) <= c, "too many live vertices for W / c: raise W or lower live_frac"
            at = k * c + rng.choice(c, len(piece), replace=False)
            kind[at] = 0
            tail[at] = piece
    kind = np.resize(kind, n)                                 # the layout repeats with period W
    tail = np.resize(tail, n)
    e1 = np.empty(n, np.int64)
    e2 = np.empty(n, np.int64)

    # ---- spine: the same tail every W positions, a fresh Zipf parent each time (ranks fixed per level)
    sp = np.flatnonzero(kind == 0)
    e1[sp] = tail[sp]
    rank_of = [rng.permutation(np.arange(start[h], start[h + 1])) for h in range(levels)]
    for h in range(1, levels):
        at = sp[lev_int[tail[sp]] == h]
        cdf = _zipf_cdf(sizes[h - 1], spine_s)
        e2[at] = rank_of[h - 1][_draw(rng, cdf, len(at))]

    # ---- D endpoints: uniform, or from a band that drifts along the stream (vertices leave the window)
    def dead_ids(pos):
        if not churn:
            return dead0 + rng.integers(0, n_dead, len(pos))
        band = max(n_dead // 8, 64)
        lo = (pos * (n_dead - band) // max(n - 1, 1)).astype(np.int64)
        return dead0 + lo + rng.integers(0, band, len(pos))

    # ---- fan: L tails of the chunk's parity (Zipf, top out-degree ~ fan_max), D heads; some repeat the previous fan edge
    fan = np.flatnonzero(kind == 1)
    if parents_in_frontier:
        groups = [(fan, np.arange(n_live))]
    else:
        groups = [(fan[chunk_par[fan] == par], np.flatnonzero(lev_int[:n_live] % 2 == par)) for par in (0, 1)]
    for at, pool in groups:
        pool = rng.permutation(pool)
        per_window = max(1, len(at) * W // n)
        cdf = _zipf_cdf(len(pool), _zipf_for_top_share(len(pool), min(0.9, fan_max / per_window)))
        e1[at] = pool[_draw(rng, cdf, len(at))]
    e2[fan] = dead_ids(fan)
    prev_fan = np.zeros(n, bool)
    prev_fan[1:] = (kind[:-1] == 1) & (np.arange(1, n) % c != 0)
    dup = fan[(rng.random(len(fan)) < dup_frac) & prev_fan[fan]]
    e1[dup] = e1[dup - 1]
    e2[dup] = e2[dup - 1]

    # ---- dead: D -> D, no self-loops
    dd = np.flatnonzero(kind == 2)
    e1[dd] = dead_ids(dd)
    e2[dd] = dead_ids(dd)
    same = e1[dd] == e2[dd]
    e2[dd[same]] = dead0 + (e2[dd[same]] - dead0 + 1) % n_dead

    # ---- external ids
    perm = rng.permutation(V).astype(np.int64)                # internal -> external
    level = np.empty(V, np.int32)
    level[perm] = lev_int
    x1, x2 = perm[e1].astype(np.int32), perm[e2].astype(np.int32)
    # sources: the roots, then the level-1 vertices ranked by their subtree in the initial window
    par0 = np.full(V, -1, np.int64)
    par0[e1[:W][kind[:W] == 0]] = e2[:W][kind[:W] == 0]
    sub = np.ones(V, np.int64)
    for h in range(levels - 1, 1, -1):
        vs = np.flatnonzero((lev_int == h) & (par0 >= 0))
        np.add.at(sub, par0[vs], sub[vs])
    l1 = np.arange(start[1], start[2])
    l1 = l1[np.lexsort((l1, -sub[l1]))]
    sources = np.concatenate([np.arange(start[0], start[1]), l1])
    parent = np.full(n, -1, np.int32)
    parent[sp] = perm[e2[sp]]
    meta = dict(level=level, kind=kind.astype(np.int8), parent=parent, sources=perm[sources].astype(np.int32),
                sizes=sizes, parents_in_frontier=parents_in_frontier)
    return V, x1, x2, meta
