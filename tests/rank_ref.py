"""The ranked queries (dppr_topk_ranked / dppr_group_topk_ranked / dppr_rank_score_at, include/dppr.h) in numpy, for the tests.
The inputs are what the engine reports through its other calls: the dense columns of group_read (or read) and the out-CSR of the
epoch by external id from read_out_graph. Degrees are a np.bincount over the tails of the stored edges, a score is ONE `*` or `/`
per element (numpy rounds each to double, nothing fused), masked or excluded entries are set to +0.0, and the order is the
expected() of tests/test_weighted_gpu.py: score > min_score, score descending, id ascending."""
import numpy as np

from tests.test_weighted_gpu import expected

NONE, DEV, DEG, INV_DEG = 0, 1, 2, 3
SEEDS, IN_NEIGHBOURS, OUT_NEIGHBOURS = 1, 2, 4


def edges(row, col):
    """(tails, heads) of the stored edges from an out-CSR by external id (duplicates kept)."""
    row = np.asarray(row, dtype=np.int64)
    V = len(row) - 1
    return np.repeat(np.arange(V, dtype=np.int64), np.diff(row)), np.asarray(col, dtype=np.int64)[:row[-1]]


def out_degree(V, tails):
    return np.bincount(tails, minlength=V).astype(np.int64)


def excluded(V, tails, heads, seeds, exclude):
    """Per lane the vertices excluded for it: a bool [n][V]. seeds: one id array per lane."""
    out = np.zeros((len(seeds), V), dtype=bool)
    for i, s in enumerate(seeds):
        s = np.atleast_1d(np.asarray(s, dtype=np.int64))
        is_seed = np.zeros(V, dtype=bool)
        is_seed[s] = True
        if exclude & SEEDS:
            out[i] |= is_seed
        if exclude & IN_NEIGHBOURS:  # v with a stored edge v -> seed
            out[i, tails[is_seed[heads]]] = True
        if exclude & OUT_NEIGHBOURS:  # v with a stored edge seed -> v
            out[i, heads[is_seed[tails]]] = True
    return out


def score(p, factor=NONE, outdeg=None, g=None):
    """One lane's score before mask and exclusion: one rounding per element."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        if factor == NONE:
            return p.copy()
        if factor == DEV:
            return p * np.asarray(g).astype(np.float64)  # (f32 -> f64 is exact)
        d = (np.asarray(outdeg, dtype=np.int64) + 1).astype(np.float64)
        return p * d if factor == DEG else p / d


def scores(cols, factor=NONE, outdeg=None, g=None, allow=None, deny=None, excl=None):
    """The score of every lane by external id: a list of [V] arrays. cols: the dense p of every lane; allow / deny: [V] masks
    (nonzero = set); excl: the bool [n][V] of excluded()."""
    res = []
    for i, p in enumerate(cols):
        s = score(p, factor, outdeg, g)
        gone = np.zeros(len(s), dtype=bool)
        if allow is not None:
            gone |= np.asarray(allow) == 0
        if deny is not None:
            gone |= np.asarray(deny) != 0
        if excl is not None:
            gone |= excl[i]
        s[gone] = 0.0
        res.append(s)
    return res


def topk(s, k, min_score=0.0):
    """(ids, scores) of one lane's order."""
    with np.errstate(all="ignore"):
        return expected(s, k, min_score)
