"""The fold of dppr_dot_dense_dev / dppr_dot_sparse (include/dppr.h) in numpy, for the tests: terms in blocks of 2^16 slots, a block
summed by the balanced tree that adds neighbours (padding +0.0), the blocks added in ascending order."""
import numpy as np

B = 1 << 16


def fold_stated(t):
    """t[..., slots] -> [...]: the definition word for word (every block padded to 2^16 slots)."""
    t = np.asarray(t, dtype=np.float64)
    m = t.shape[-1]
    if m == 0:
        return np.zeros(t.shape[:-1])
    nb = -(-m // B)
    y = np.concatenate([t, np.zeros(t.shape[:-1] + (nb * B - m,))], -1).reshape(t.shape[:-1] + (nb, B))
    while y.shape[-1] > 1:
        y = y[..., 0::2] + y[..., 1::2]
    y = y[..., 0]
    acc = y[..., 0].copy()
    for b in range(1, nb):
        acc = acc + y[..., b]
    return acc


def _block(t):
    """One block of 1 .. 2^16 slots: the tree over the next power of two, then the sums of pure padding (each exactly +0.0)
    added level by level -- the same bits as padding the block out, without the 2^16 columns."""
    m = t.shape[-1]
    m2 = 1
    while m2 < m:
        m2 *= 2
    y = np.concatenate([t, np.zeros(t.shape[:-1] + (m2 - m,))], -1)
    while y.shape[-1] > 1:
        y = y[..., 0::2] + y[..., 1::2]
    y = y[..., 0]
    while m2 < B:
        y = y + 0.0
        m2 *= 2
    return y


def fold(t):
    """t[..., slots] -> [...]: fold_stated, bit for bit (tests/test_dot_plan.py holds the two together)."""
    t = np.asarray(t, dtype=np.float64)
    m = t.shape[-1]
    if m == 0:
        return np.zeros(t.shape[:-1])
    acc = _block(t[..., :B])
    for a in range(B, m, B):
        acc = acc + _block(t[..., a:a + B])
    return acc


def dense(h, cols):
    """h [F][V] (f64), cols: the n dense reads -> [F][n]"""
    x = np.stack(cols, axis=1)  # [V][n]
    return fold(np.asarray(h, dtype=np.float64)[:, None, :] * x.T[None, :, :])


def sparse(offsets, ids, w, cols):
    """One CSR over the queries -> [F][n]"""
    x = np.stack(cols, axis=1)
    out = np.zeros((len(offsets) - 1, x.shape[1]))
    for f in range(len(offsets) - 1):
        a, b = int(offsets[f]), int(offsets[f + 1])
        out[f] = fold(np.asarray(w[a:b], dtype=np.float64)[None, :] * x[np.asarray(ids[a:b], dtype=np.int64)].T)
    return out


def running(t):
    """The slot-by-slot running sum: what the fold is NOT."""
    acc = 0.0
    for v in np.asarray(t, dtype=np.float64):
        acc = acc + v
    return acc
