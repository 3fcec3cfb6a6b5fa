"""The numpy restatement of dppr_assign / dppr_assign_at (include/dppr.h) from the dense group_read of every named group: one
multiplication per score, the first maximum, the runner-up and the margin by the operations of the definition, the counts and the
flips. Nothing here touches a device."""
import numpy as np


def dense(engine, groups):
    """[V][C] p of the classes of a call: the lanes of `groups` (handles of `engine`, n lanes each as a dict or a callable), in
    call order, each column exactly what group_read returns."""
    cols = []
    for g in groups:
        for i in range(engine._group_n[g]):
            cols.append(engine.group_read(g, i)[0])
    return np.ascontiguousarray(np.stack(cols, axis=1))


def scores(p, scale=None):
    """score_c[v] = scale[c] * p_c[v], one multiplication; scale None: p itself."""
    p = np.asarray(p, dtype=np.float64)
    return p if scale is None else p * np.asarray(scale, dtype=np.float64)[None, :]


def assign(p, scale=None, min_score=0.0):
    """(label, best, second, second_label, margin) of every row of p ([V][C])."""
    s = scores(p, scale)
    V, C = s.shape
    rows = np.arange(V)
    cand = np.where(s > min_score, s, -np.inf)          # (a NaN never qualifies: `>` is false)
    first = np.argmax(cand, axis=1)                     # (the first maximum)
    has = cand[rows, first] > -np.inf
    label = np.where(has, first, -1).astype(np.int32)
    best = np.where(has, s[rows, first], 0.0)
    second = np.zeros(V)                                # starts at +0.0
    second_label = np.full(V, -1, dtype=np.int32)
    for c in range(C):                                  # replaced only by a strictly greater score of a class other than label
        take = (label != c) & (s[:, c] > second)
        second = np.where(take, s[:, c], second)
        second_label = np.where(take, c, second_label).astype(np.int32)
    margin = np.where(has, best - second, 0.0)
    return label, best, second, second_label, margin


def counts(label, C):
    """int64 [C + 1]: vertices labelled c, then the unassigned."""
    out = np.zeros(C + 1, dtype=np.int64)
    for c in range(C):
        out[c] = np.count_nonzero(label == c)
    out[C] = np.count_nonzero(label == -1)
    return out


def flips(prev, label):
    """(id, old, new) int32 of the ids whose label changed, ascending by id."""
    prev, label = np.asarray(prev, dtype=np.int32), np.asarray(label, dtype=np.int32)
    ids = np.nonzero(prev != label)[0].astype(np.int32)
    return ids, prev[ids].copy(), label[ids].copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
