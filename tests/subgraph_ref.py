"""The induced subgraph of dppr_subgraph / dppr_group_subgraph (include/dppr.h) in numpy, for the tests. The inputs are what the
engine reports through its other calls: the order from topk / group_topk, the rows of the out-CSR by external id from
read_out_graph. Row j is the sorted positions of the heads of v_j's stored out-edges that lie in the order, duplicates kept, a self
loop included."""
import numpy as np


def rows(V, row_ptr, col, order):
    """The rows of one source: a list of L int32 arrays."""
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    order = np.asarray(order, dtype=np.int64)
    L = len(order)
    assert len(np.unique(order)) == L
    pos = np.full(V, -1, dtype=np.int64)
    pos[order] = np.arange(L)
    out = []
    for v in order:
        r = pos[col[row_ptr[v]:row_ptr[v + 1]]]
        out.append(np.sort(r[r >= 0]).astype(np.int32))
    return out


def brute_rows(V, row_ptr, col, order):
    """The same by a double loop over the positions: for small graphs."""
    order = [int(v) for v in order]
    out = []
    for v in order:
        heads = [int(w) for w in col[row_ptr[v]:row_ptr[v + 1]]]
        out.append(np.array([b for b, w in enumerate(order) for h in heads if h == w], dtype=np.int32))
    return out


def subgraph(V, row_ptr, col, orders, k):
    """What the engine returns for the sources whose top-k orders are `orders` (each already cut to k): (counts [n], offsets [n + 1],
    ids [n][k], row_ptr [n][k + 1], col), ids -1 past the count, row_ptr absolute."""
    n = len(orders)
    counts = np.array([len(o) for o in orders], dtype=np.int32)
    ids = np.full((n, k), -1, dtype=np.int32)
    rp = np.zeros((n, k + 1), dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    cols = []
    for i, order in enumerate(orders):
        L = len(order)
        assert L <= k
        ids[i, :L] = order
        rs = rows(V, row_ptr, col, order)
        lens = np.array([len(r) for r in rs], dtype=np.int64)
        rp[i, :L + 1] = offsets[i] + np.concatenate([[0], np.cumsum(lens)])
        rp[i, L + 1:] = rp[i, L]
        offsets[i + 1] = rp[i, L]
        cols += rs
    return counts, offsets, ids, rp, (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)
