"""dppr_forward_push (include/dppr.h) in numpy, word for word, for the tests, on forward_ref.Rows (the in-rows in the order the
device stores them). Every round is the DENSE one of the definition: the comparison, the push, and the gather over every row as
dot_ref.fold; the device may skip rows, the definition does not. Everything is by external id; a column is computed on its own."""
import numpy as np

from tests import dot_ref
from tests.forward_ref import ALPHA, DAMP


def rowless_mask(rows):
    """The vertices without a row: those that no stored edge names (a vertex without an internal id and a parked one among them)."""
    return (np.diff(rows.ptr) == 0) & (rows.d == 0)


class Column:
    """One column: p, r [V], rounds_used, converged, rem, pushes, left, and fronts = the frontier of every round that pushed."""


def push(rows, rowless, ids, weights, eps, max_rounds):
    assert 1 <= max_rounds <= 256 and eps > 0.0
    ids, weights = np.atleast_1d(np.asarray(ids, dtype=np.int64)), np.atleast_1d(np.asarray(weights, dtype=np.float64))
    assert len(ids) == len(weights) >= 1 and len(np.unique(ids)) == len(ids) and np.all(weights > 0)
    p, r = np.zeros(rows.V), np.zeros(rows.V)
    has_row = ~rowless[ids]
    r[ids[has_row]] = weights[has_row]
    den = rows.d + 1.0
    thr = eps * den
    c = Column()
    c.fronts, c.pushes = [], 0
    for _ in range(max_rounds):
        F = r > thr
        if not F.any():
            break
        p[F] = p[F] + ALPHA * r[F]
        y = np.zeros(rows.V)
        y[F] = (DAMP * r[F]) / den[F]
        r[F] = 0.0
        r = r + rows.pull(y)
        c.fronts.append(F)
        c.pushes += int(F.sum())
    c.rounds_used = len(c.fronts)
    c.left = int(np.sum(r > thr))
    c.converged = int(c.left == 0)
    c.rem = float(dot_ref.fold(r))
    p[ids[~has_row]] = ALPHA * weights[~has_row]   # settled exactly: no round, no statistic
    c.p, c.r = p, r
    return c


def work(rows, columns):
    """[rows pushed, rows gathered, their in-edges] over the union of the columns' frontiers per round, summed over the rounds."""
    out = np.zeros(3, dtype=np.int64)
    length = np.diff(rows.ptr)
    for k in range(max(c.rounds_used for c in columns)):
        U = np.zeros(rows.V, dtype=bool)
        for c in columns:
            if k < c.rounds_used:
                U |= c.fronts[k]
        recv = np.unique(rows.heads[U[rows.tails]])
        out += (int(U.sum()), len(recv), int(length[recv].sum()))
    return out


def gathered_per_round(rows, column):
    """Rows gathered in each round of one column alone."""
    return [len(np.unique(rows.heads[F[rows.tails]])) for F in column.fronts]
