"""The forward walk of dppr_walks / dppr_refine_at (include/dppr.h) in numpy, for the tests: Philox4x32-10 keyed by the seed with
counter (w, v, t, 0), stop below floor(0.15 * 2^32), one of outdeg + 1 choices of which the last is death, at most 256 steps. All
walks of a call advance together, one step a pass; a walk is a function of (start external id, walk number, seed) and of the rows
alone, so the order they are run in changes nothing."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
STOP_BELOW = 0x26666666
MAX_STEPS = 256
U32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Counters: arrays (or scalars) of values below 2^32; key: two Python ints. Four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & U32 for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & U32, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & U32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def pick(x1, x2, d):
    """floor(((x1 * 2^32 + x2) * (d + 1)) / 2^64) without 128-bit integers: d + 1 < 2^32, so neither product overflows 64 bits."""
    n = np.asarray(d, dtype=np.uint64) + np.uint64(1)
    return (x1 * n + ((x2 * n) >> S32)) >> S32


def internal_csr(V, ext_row, ext_col, ext2int):
    """The rows the device holds, from dppr_read_out_graph (rows by external id) and dppr_debug_id_map: rows by internal id,
    neighbours as internal ids in ascending order, duplicates kept. Returns (row_ptr [V + 1], col, int2ext [V], -1 where no vertex)."""
    ext2int = np.asarray(ext2int, dtype=np.int64)
    int2ext = np.full(V, -1, dtype=np.int64)
    have = np.nonzero(ext2int >= 0)[0]
    int2ext[ext2int[have]] = have
    ext_row, ext_col = np.asarray(ext_row, dtype=np.int64), np.asarray(ext_col, dtype=np.int64)
    ext_deg = np.diff(ext_row)
    assert np.all(ext_deg[ext2int < 0] == 0)
    tail, head = ext2int[np.repeat(np.arange(V), ext_deg)], ext2int[ext_col[:ext_row[-1]]]
    order = np.lexsort((head, tail))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(tail, minlength=V))])
    col = head[order]
    return row_ptr, col, int2ext


def walks(row_ptr, col, ext2int, int2ext, starts, W, seed, with_steps=False):
    """Endpoints [m][W] (external id, -1 for a walk that died) of W walks from each external id of `starts`."""
    starts = np.asarray(starts, dtype=np.int64)
    m = len(starts)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    v = np.repeat(starts, W)
    w = np.tile(np.arange(W, dtype=np.int64), m)
    u = np.asarray(ext2int, dtype=np.int64)[v]
    ends = np.full(m * W, -1, dtype=np.int64)
    steps = np.zeros(m * W, dtype=np.int64)
    alive = np.arange(m * W)
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    for t in range(MAX_STEPS):
        if len(alive) == 0:
            break
        x0, x1, x2, _ = philox(w[alive], v[alive], t, 0, k0, k1)
        steps[alive] += 1
        ua = u[alive]
        stop = x0 < np.uint64(STOP_BELOW)
        ends[alive[stop]] = np.where(ua[stop] >= 0, int2ext[np.maximum(ua[stop], 0)], v[alive[stop]])
        go = ~stop
        alive, ua, x1, x2 = alive[go], ua[go], x1[go], x2[go]
        has = ua >= 0
        rs = np.where(has, row_ptr[np.maximum(ua, 0)], 0)
        d = np.where(has, row_ptr[np.maximum(ua, 0) + 1] - rs, 0)
        j = pick(x1, x2, d).astype(np.int64)
        on = j < d  # (j == d: the death slot; the endpoint stays -1)
        alive = alive[on]
        u[alive] = col[rs[on] + j[on]]
    ends = ends.reshape(m, W).astype(np.int32)
    return (ends, steps.reshape(m, W)) if with_steps else ends


def terms(ends, r_cols):
    """t[i][q][w] = r_i[X_w], +0.0 for a walk that died: r_cols the n dense reads by external id."""
    ends = np.asarray(ends, dtype=np.int64)
    r = np.stack(r_cols, axis=0)  # [n][V]
    return np.where(ends[None, :, :] >= 0, r[:, np.maximum(ends, 0)], 0.0)


def hoeffding(R, W, delta=1e-12):
    """|mean of W terms in [-R, R] - its expectation| <= this with probability 1 - delta, plus the bias budget 1e-8 R."""
    return R * np.sqrt(2.0 * np.log(2.0 / delta) / W) + 1e-8 * R
