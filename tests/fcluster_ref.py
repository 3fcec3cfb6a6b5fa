"""The full-length conductance sweep of a forward track (dppr_ftrack_cluster, include/dppr.h) in numpy, for the tests. The inputs
are a column's p by external id (tests/ftrack_ref.py) and the epoch's out-rows by external id (read_out_graph, or built from the
stored edges). The qualifying set and the order are stated here; the prefix arrays and the best prefix are
tests/cluster_ref.prefix_arrays / best unchanged -- the SET definition, not the per-position differences the kernels sum."""
import numpy as np

from tests import cluster_ref as cr

BY_P, BY_P_OVER_DEG = 0, 1
ORDERS = {"p": BY_P, "deg": BY_P_OVER_DEG}


def out_rows(V, tails, heads):
    """(row_ptr, col) of the stored edges tail -> head by external id, duplicates kept."""
    tails, heads = np.asarray(tails, dtype=np.int64), np.asarray(heads, dtype=np.int64)
    o = np.argsort(tails, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(tails, minlength=V))]).astype(np.int64), heads[o]


def scores(p, row_ptr, order):
    p = np.asarray(p, dtype=np.float64)
    if ORDERS.get(order, order) == BY_P:
        return p.copy()
    with np.errstate(invalid="ignore"):
        return p / (np.diff(np.asarray(row_ptr, dtype=np.int64)).astype(np.float64) + 1.0)   # ONE division


def ordered(p, row_ptr, col, order, min_score=0.0, max_len=0):
    """(ids, score) of the order: named by a stored edge, score > min_score, score descending, external id ascending."""
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)[:int(row_ptr[-1])]
    V = len(row_ptr) - 1
    s = scores(p, row_ptr, order)
    named = (np.diff(row_ptr) > 0) | (np.bincount(col, minlength=V) > 0)
    with np.errstate(invalid="ignore"):
        ids = np.nonzero(named & (s > min_score))[0]
    ids = ids[np.lexsort((ids, -s[ids]))]
    if max_len:
        ids = ids[:max_len]
    return ids.astype(np.int32), s[ids]


def cluster(p, row_ptr, col, order, min_score=0.0, max_len=0, min_size=1):
    """What the engine returns for one column: (best dict, ids, score, cut_out, cut_in, vol)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    V, Ed = len(row_ptr) - 1, int(row_ptr[-1])
    ids, s = ordered(p, row_ptr, col, order, min_score, max_len)
    co, ci, vol = cr.prefix_arrays(V, row_ptr, col, ids)
    return cr.best(co, vol, Ed, min_size), ids, s, co, ci, vol


def same(got, want, what=""):
    """got: (best, ids, score, cut_out, cut_in, vol) of one column from the engine; compared as integers and by bit pattern."""
    gb, wb = dict(got[0]), dict(want[0])
    assert np.float64(gb.pop("best_phi")).view(np.uint64) == np.float64(wb.pop("best_phi")).view(np.uint64), (what, got[0], want[0])
    assert gb == wb, (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, "ids", got[1][:8], want[1][:8], len(got[1]), len(want[1]))
    assert np.array_equal(np.asarray(got[2]).view(np.uint64), np.asarray(want[2], dtype=np.float64).view(np.uint64)), (what, "score")
    for k, name in ((3, "cut_out"), (4, "cut_in"), (5, "vol")):
        assert np.array_equal(got[k], want[k]), (what, name)
