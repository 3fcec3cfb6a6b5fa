"""dppr_certify / dppr_group_certify (include/dppr.h) in numpy, for the tests: the residual norms of every lane -- counts, the
largest |r| with the smallest id that attains it, the two sums in the fold of the dot family (tests/dot_ref.py) -- and the largest
violation of the loop invariant over a list of directed edges. States are dense reads by EXTERNAL id, one [V] array per lane.

The sums inside the invariant are numpy's (np.bincount adds an out-row's heads in the order of the edge list); the device adds them
in its own order, so inv_max_err agrees to rounding, not to the bit, and inv_argmax only where the maximum stands clear."""
import numpy as np

from tests import dot_ref

ALPHA = 0.15
ONE_MINUS_ALPHA = 1.0 - 0.15


def seed_vector(V, seed):
    """h of a lane: the indicator of a source (an int), the weights of a set lane (a list of (id, weight)), zeros for None."""
    h = np.zeros(V)
    if seed is None:
        return h
    if np.isscalar(seed):
        h[int(seed)] = 1.0
        return h
    for v, w in seed:
        h[int(v)] = float(w)
    return h


def _max_and_first(x, take):
    """The largest x among the rows `take` and the smallest index that attains it; (0.0, -1) if there is none."""
    idx = np.nonzero(take)[0]
    if len(idx) == 0:
        return 0.0, -1
    m = float(np.max(x[idx]))
    return m, int(idx[np.nonzero(x[idx] == m)[0][0]])


def residual(p_cols, r_cols, eps, has_id=None):
    """The residual part. has_id [V]: which vertices have an internal id (default: all of them) -- a vertex without one holds
    p = r = 0 and takes no part, which shows only where a maximum is 0.0."""
    n, V = len(p_cols), len(p_cols[0])
    has_id = np.ones(V, dtype=bool) if has_id is None else np.asarray(has_id, dtype=bool)
    out = {"max_abs_r": np.zeros(n), "argmax_r": np.zeros(n, dtype=np.int32), "sum_abs_r": np.zeros(n), "sum_p": np.zeros(n),
           "n_pos": np.zeros(n, dtype=np.int64), "n_neg": np.zeros(n, dtype=np.int64), "n_nonfinite": np.zeros(n, dtype=np.int64),
           "n_p_nonzero": np.zeros(n, dtype=np.int64)}
    for i in range(n):
        p, r = np.asarray(p_cols[i], dtype=np.float64), np.asarray(r_cols[i], dtype=np.float64)
        bad = has_id & ~(np.isfinite(p) & np.isfinite(r))
        ok = has_id & ~bad
        pz, rz = np.where(ok, p, 0.0), np.where(ok, np.abs(r), 0.0)   # (a row that is not finite: +0.0 in both sums)
        out["n_nonfinite"][i] = int(bad.sum())
        out["n_pos"][i] = int((ok & (np.where(ok, r, 0.0) > eps)).sum())
        out["n_neg"][i] = int((ok & (np.where(ok, r, 0.0) < -eps)).sum())
        out["n_p_nonzero"][i] = int((ok & (pz != 0.0)).sum())
        out["max_abs_r"][i], out["argmax_r"][i] = _max_and_first(rz, ok)
        out["sum_abs_r"][i] = dot_ref.fold(rz)
        out["sum_p"][i] = dot_ref.fold(pz)
    return out


def invariant_err(V, tails, heads, p, r, seed):
    """err[u] = |(p[u] + 0.15 r[u]) - (0.15 h[u] + (0.85 S[u]) / (d(u) + 1))| over the stored edges tails -> heads (duplicates and
    self loops as stored), every operation rounded where it stands."""
    tails, heads = np.asarray(tails, dtype=np.int64), np.asarray(heads, dtype=np.int64)
    p, r = np.asarray(p, dtype=np.float64), np.asarray(r, dtype=np.float64)
    d = np.bincount(tails, minlength=V)
    with np.errstate(invalid="ignore", over="ignore"):
        S = np.bincount(tails, weights=p[heads], minlength=V)
        lhs = p + ALPHA * r
        rhs = ALPHA * seed_vector(V, seed) + (ONE_MINUS_ALPHA * S) / (d + 1.0)
        return np.abs(lhs - rhs)


def invariant(V, tails, heads, p_cols, r_cols, seeds, has_id=None):
    """The invariant part: inv_max_err, inv_argmax [n] and the errors themselves, err [n][V]. An err that is not finite takes no part."""
    n = len(p_cols)
    has_id = np.ones(V, dtype=bool) if has_id is None else np.asarray(has_id, dtype=bool)
    out = {"inv_max_err": np.zeros(n), "inv_argmax": np.zeros(n, dtype=np.int32), "err": np.zeros((n, V))}
    for i in range(n):
        err = invariant_err(V, tails, heads, p_cols[i], r_cols[i], seeds[i])
        take = has_id & np.isfinite(err)
        out["err"][i] = err
        out["inv_max_err"][i], out["inv_argmax"][i] = _max_and_first(np.where(take, err, 0.0), take)
    return out


def certify(V, tails, heads, p_cols, r_cols, seeds, eps, has_id=None):
    """Both parts in one dict (the keys of Engine.group_certify, and err [n][V])."""
    out = residual(p_cols, r_cols, eps, has_id)
    out.update(invariant(V, tails, heads, p_cols, r_cols, seeds, has_id))
    return out
