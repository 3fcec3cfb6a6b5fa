"""The sampler of dppr_sample / dppr_group_sample (include/dppr.h) in numpy, for the tests: the weight rule, the balanced sum
tree over the weights in external-id order, the uniform of draw number j of lane i (the Philox4x32-10 of tests/walk_ref.py with
counter (lo32 j, hi32 j, i, 0x53414D50)) and the descent, vectorised over the draws and looping over the levels. Every step is
one IEEE addition, subtraction, multiplication or comparison, so the device's draws are these bit for bit."""
import numpy as np

from tests import walk_ref

DOMAIN = 0x53414D50
OK, EMPTY, NONFINITE = 0, 1, 2
MASK64 = (1 << 64) - 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def weights(score, min_score=0.0):
    """w = score where score > min_score, +0.0 elsewhere (a NaN, a negative or a zero score weighs nothing)."""
    score = np.asarray(score, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(score > min_score, score, 0.0)


def tree(w):
    """The levels of the tree over P leaves, P the smallest power of two >= len(w): [leaves, ..., [root]]."""
    w = np.asarray(w, dtype=np.float64)
    P = 1
    while P < len(w):
        P *= 2
    y = np.zeros(P, dtype=np.float64)
    y[:len(w)] = w
    levels = [y]
    with np.errstate(invalid="ignore", over="ignore"):
        while len(y) > 1:
            y = y[0::2] + y[1::2]
            levels.append(y)
    return levels


def status(root):
    if root == 0.0:
        return EMPTY
    return OK if np.isfinite(root) else NONFINITE


def uniforms(lane, seed, first, S):
    """u of the draws number first .. first + S - 1 of lane `lane`: float64 [S] in [0, 1)."""
    j = [(int(first) + t) & MASK64 for t in range(int(S))]
    lo = np.array([x & 0xFFFFFFFF for x in j], dtype=np.uint64)
    hi = np.array([x >> 32 for x in j], dtype=np.uint64)
    if S == 0:
        return np.zeros(0, dtype=np.float64)
    x0, x1, _, _ = walk_ref.philox(lo, hi, np.full(S, lane, dtype=np.uint64), np.full(S, DOMAIN, dtype=np.uint64),
                                   int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    m = ((x0 << np.uint64(32)) | x1) >> np.uint64(11)
    return m.astype(np.float64) * 2.0 ** -53


def descend(levels, x):
    """The leaf of every x (already scaled by the root): int64 [len(x)]."""
    x = np.array(x, dtype=np.float64)
    k = np.zeros(len(x), dtype=np.int64)
    for l in range(len(levels) - 1, 0, -1):
        L, R = levels[l - 1][2 * k], levels[l - 1][2 * k + 1]
        right = (x >= L) & (R > 0.0)
        x = np.where(right, x - L, x)
        k = 2 * k + right
    return k


def draw(levels, lane, seed, first, S):
    """(ids int32 [S], w float64 [S]) of lane `lane` over its tree; -1 and +0.0 where the root is zero or not finite."""
    root = levels[-1][0]
    if status(root) != OK:
        return np.full(S, -1, dtype=np.int32), np.zeros(S, dtype=np.float64)
    k = descend(levels, uniforms(lane, seed, first, S) * root)
    return k.astype(np.int32), levels[0][k]


def group_sample(scores, S, min_score=0.0, seed=0, first=0):
    """The whole call over scores [V][n] (lane i = column i): (ids [n][S], w [n][S], total [n], support [n], status [n])."""
    scores = np.asarray(scores, dtype=np.float64)
    n = scores.shape[1]
    ids, w = np.empty((n, S), dtype=np.int32), np.empty((n, S), dtype=np.float64)
    total, support, stat = np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    for i in range(n):
        lv = tree(weights(scores[:, i], min_score))
        ids[i], w[i] = draw(lv, i, seed, first, S)
        total[i], support[i], stat[i] = lv[-1][0], np.count_nonzero(lv[0] > 0.0), status(lv[-1][0])
    return ids, w, total, support, stat
