"""The forward track (dppr_ftrack_*, include/dppr.h) in numpy, word for word, for the tests: one column's (p, r) by external id,
created on an epoch as tests/fpush_ref.py pushes, then moved from epoch to epoch by the fix-up over the batch's records (steps T and
H) and the SIGNED rounds. Rows are forward_ref.Rows of each epoch; the records are those of SlidingStream.batch_arrays() (tail,
head, is_insert), the mirrored copies of an undirected window among them. Every round is the DENSE one of the definition."""
import numpy as np

from tests import dot_ref
from tests import fpush_ref as pr
from tests.forward_ref import ALPHA, DAMP


class Call:
    """What one create or update call reports for a column: rounds_used, converged, rem, pushes, left, fronts (the frontier of every
    round that pushed, for fpush_ref.work) and fix = [records applied, distinct tails, distinct heads]."""


def fixup(p, r, d1, tails, heads, ins):
    """Steps T and H over the L records of the batch that made the epoch whose stored out-degrees are d1. Returns new (p, r)."""
    p, r = p.copy(), r.copy()
    tails, heads = np.asarray(tails, dtype=np.int64), np.asarray(heads, dtype=np.int64)
    ins = np.asarray(ins).astype(bool)
    V = len(p)
    ut = np.unique(tails)
    n_ins = np.bincount(tails[ins], minlength=V)[ut].astype(np.float64)
    n_del = np.bincount(tails[~ins], minlength=V)[ut].astype(np.float64)
    d1u = np.asarray(d1, dtype=np.float64)[ut]
    d0 = d1u - n_ins + n_del
    assert np.all(d0 >= 0)
    g = p[ut] / (ALPHA * (d0 + 1.0))          # from p before any change
    c = np.zeros(V)
    c[ut] = DAMP * g
    ch = d1u != d0
    u = ut[ch]
    p[u] = (p[u] * (d1u[ch] + 1.0)) / (d0[ch] + 1.0)
    r[u] = r[u] - (d1u[ch] - d0[ch]) * g[ch]
    for i in range(len(tails)):                # step H: ascending i, one rounding per record
        w = heads[i]
        r[w] = r[w] + c[tails[i]] if ins[i] else r[w] - c[tails[i]]
    return p, r


class Column:
    """One column of a track: ids / weights / eps, the state p, r [V] and `last`, the Call of the last create or update."""

    def __init__(self, rows, ids, weights, eps, max_rounds):
        ids, weights = np.atleast_1d(np.asarray(ids, dtype=np.int64)), np.atleast_1d(np.asarray(weights, dtype=np.float64))
        assert len(ids) == len(weights) >= 1 and len(np.unique(ids)) == len(ids) and np.all(weights > 0) and eps > 0.0
        self.ids, self.weights, self.eps = ids, weights, float(eps)
        rowless = pr.rowless_mask(rows)
        has_row = ~rowless[ids]
        self.p, self.r = np.zeros(rows.V), np.zeros(rows.V)
        self.r[ids[has_row]] = weights[has_row]
        self._rounds(rows, max_rounds, [0, 0, 0])
        self.p[ids[~has_row]] = ALPHA * weights[~has_row]   # settled exactly: no round, no statistic

    def _rounds(self, rows, max_rounds, fix):
        assert 1 <= max_rounds <= 256
        p, r = self.p, self.r
        den = rows.d + 1.0
        thr = self.eps * den
        c = Call()
        c.fronts, c.pushes, c.fix = [], 0, list(fix)
        for _ in range(max_rounds):
            F = np.abs(r) > thr
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
        c.left = int(np.sum(np.abs(r) > thr))
        c.converged = int(c.left == 0)
        c.rem = float(dot_ref.fold(np.abs(r)))
        assert not np.any(np.signbit(r) & (r == 0.0))   # r is never -0.0
        self.p, self.r, self.last = p, r, c

    def update(self, rows, records, max_rounds):
        """To the epoch of `rows`: records = (tails, heads, ins) of its batch, or None for more rounds on the track's own epoch."""
        fix = [0, 0, 0]
        if records is not None:
            tails, heads, ins = records
            self.p, self.r = fixup(self.p, self.r, rows.d, tails, heads, ins)
            fix = [len(tails), len(np.unique(tails)), len(np.unique(heads))]
        self._rounds(rows, max_rounds, fix)
        return self.last


def work(rows, calls):
    """fpush_ref.work over the last calls of a track's columns."""
    if max(c.rounds_used for c in calls) == 0:
        return np.zeros(3, dtype=np.int64)
    return pr.work(rows, calls)
