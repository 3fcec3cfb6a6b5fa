"""The position queries (dppr_position_at / dppr_group_position_at, include/dppr.h) in numpy, for the tests. The scores are those of
tests/rank_ref.py (rank_ref.scores over the dense columns and the out-CSR the engine reports). A lane's order is np.lexsort over
(id, -score) among score > min_score; a position is the inverse of that permutation, -1 for what is not in it; the count is its
length. Every number is an integer defined by comparisons alone."""
import numpy as np

from tests import rank_ref

scores = rank_ref.scores   # THE SCORE is the ranked family's, unchanged


def order(s, min_score=0.0):
    """The external ids of one lane's whole order."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = np.nonzero(s > min_score)[0]   # (false for a NaN)
        return q[np.lexsort((q, -s[q]))]


def positions(s, ids, min_score=0.0):
    """(pos int32 [len(ids)], count) of one lane."""
    o = order(s, min_score)
    inv = np.full(len(s), -1, dtype=np.int32)
    inv[o] = np.arange(len(o), dtype=np.int32)
    return inv[np.asarray(ids, dtype=np.int64)], len(o)


def group_positions(scores, ids, min_score=0.0):
    """(pos int32 [len(ids)][n], counts int32 [n]) of the lanes whose scores are given, one [V] array each."""
    res = [positions(s, ids, min_score) for s in scores]
    pos = np.stack([p for p, _ in res], axis=1).astype(np.int32).reshape(len(np.asarray(ids)), len(scores))
    return pos, np.array([c for _, c in res], dtype=np.int32)
