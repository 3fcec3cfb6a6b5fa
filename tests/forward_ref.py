"""dppr_forward (include/dppr.h) in numpy, word for word, for the tests: the in-rows in the order the device stores them (tails
ascending by INTERNAL id, stable, duplicates and self loops as stored), the per-vertex term, the row sum and the remaining mass
as dot_ref.fold, the accumulation, the check schedule with per-column freezing. Everything is by external id; a column is computed
on its own (it depends on nothing else of a call)."""
import numpy as np

from tests import dot_ref

ALPHA, DAMP, CHECK = 0.15, 0.85, 8


class Rows:
    """The in-rows of an epoch in device order, from dppr_read_graph (the in-CSR by external id) and dppr_debug_id_map.
    A tail without an internal id cannot occur (a stored edge names both ends); order = -1 sorts it first and asserts."""

    def __init__(self, V, row_ptr, col, ext2int):
        self.V = int(V)
        row_ptr = np.asarray(row_ptr, dtype=np.int64)
        tails = np.asarray(col, dtype=np.int64)[:row_ptr[-1]]
        heads = np.repeat(np.arange(self.V, dtype=np.int64), np.diff(row_ptr))
        x2i = np.asarray(ext2int, dtype=np.int64)
        assert np.all(x2i[tails] >= 0) and np.all(x2i[heads] >= 0)
        order = np.lexsort((x2i[tails], heads))           # by head, then by the internal id of the tail; stable
        self.tails, self.heads = tails[order], heads[order]
        self.ptr = np.concatenate([[0], np.cumsum(np.bincount(heads, minlength=self.V))])
        self.d = np.bincount(tails, minlength=self.V).astype(np.float64)   # stored out-degree
        # the rows of one padded length share a matrix of entry indices (-1: padding, +0.0)
        self.classes = []
        length = np.diff(self.ptr)
        for P in sorted({1 << int(n - 1).bit_length() if n > 1 else 1 for n in length[length > 0]}):
            rows = np.nonzero((length > P // 2 if P > 1 else length > 0) & (length <= P))[0]
            idx = np.full((len(rows), P), -1, dtype=np.int64)
            for j, w in enumerate(rows):
                idx[j, :length[w]] = np.arange(self.ptr[w], self.ptr[w + 1])
            self.classes.append((rows, idx))

    @classmethod
    def from_edges(cls, V, tails, heads, ext2int=None):
        """From the stored edges tail -> head in stored order (the tests' hand-made graphs): the identity numbering unless given."""
        tails, heads = np.asarray(tails, dtype=np.int64), np.asarray(heads, dtype=np.int64)
        order = np.argsort(heads, kind="stable")
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(heads, minlength=V))])
        return cls(V, row_ptr, tails[order], np.arange(V) if ext2int is None else ext2int)

    def pull(self, y):
        """x[w] = fold of y[tail] over w's in-row in stored order."""
        x = np.zeros(self.V)
        terms = np.concatenate([y[self.tails], [0.0]])   # (index -1: the padding)
        for rows, idx in self.classes:
            x[rows] = dot_ref.fold(terms[idx])
        return x


def forward(rows, q, iters, tol):
    """One column: (f [V], rem, iters_used)."""
    assert 1 <= iters <= 256 and tol >= 0.0
    x = np.zeros(rows.V)
    x[q] = 1.0
    f = ALPHA * x
    for k in range(1, iters + 1):
        y = (DAMP * x) / (rows.d + 1.0)
        x = rows.pull(y)
        f = f + ALPHA * x
        if k == iters or k % CHECK == 0:
            rem = float(dot_ref.fold(x))
            if rem <= tol or k == iters:
                return f, rem, k
    raise AssertionError("unreachable")


def topk(f, k, min_f=0.0):
    """(ids, f): f > min_f, f descending, ties by id ascending, at most k."""
    ids = np.nonzero(f > min_f)[0]
    order = np.lexsort((ids, -f[ids]))[:k]
    return ids[order].astype(np.int32), f[ids[order]]


def exact(V, tails, heads, q):
    """pihat_q by a dense solve of (I - M^T) pi = 0.15 e_q (small graphs only): to rounding, not bit for bit."""
    tails, heads = np.asarray(tails, dtype=np.int64), np.asarray(heads, dtype=np.int64)
    d = np.bincount(tails, minlength=V).astype(np.float64)
    M = np.zeros((V, V))
    np.add.at(M, (tails, heads), DAMP / (d[tails] + 1.0))
    e = np.zeros(V)
    e[q] = ALPHA
    return np.linalg.solve(np.eye(V) - M.T, e)
