"""The patch feed restated in numpy (include/dppr.h: dppr_patch / dppr_group_patch): the classification from two dense reads, the
CSR layout, the merge into a replica and the three re-mark rules on a dense mark. Everything is per lane over dense columns of V
doubles by external id; nothing here knows the engine."""
import numpy as np

KEEP_MARK, REMARK_ALL, REMARK_EMITTED = 0, 1, 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def classify(p, m, tau, delta):
    """(upsert, delete, suppressed) boolean columns of one lane. NaN and -0.0 fail `>`; |d| == delta is suppressed."""
    p, m = np.asarray(p, dtype=np.float64), np.asarray(m, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        now, then = p > tau, m > tau
        moved = np.abs(p - m) > delta  # one subtraction, rounded to nearest even
    up = now & (~then | moved)
    return up, then & ~now, now & then & ~moved


def patch(ps, ms, tau, delta):
    """ps / ms: the dense columns of every lane now and at the mark. The patch as the dict Engine.group_patch returns."""
    n = len(ps)
    uo, do = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    ui, up, di = [], [], []
    for i in range(n):
        u, d, _ = classify(ps[i], ms[i], tau, delta)
        ids = np.nonzero(u)[0]
        ui.append(ids.astype(np.int32))
        up.append(np.asarray(ps[i], dtype=np.float64)[ids])
        di.append(np.nonzero(d)[0].astype(np.int32))
        uo[i + 1], do[i + 1] = uo[i] + len(ids), do[i] + len(di[-1])
    return {"up_offsets": uo, "up_ids": np.concatenate(ui), "up_p": np.concatenate(up), "del_offsets": do, "del_ids": np.concatenate(di)}


def kinds(ps, ms, tau, delta):
    """How many entries of each of the four kinds the reference shows over all lanes: an upsert of a new entry, an upsert of a
    changed entry, a delete, an entry suppressed by delta."""
    new = changed = deleted = suppressed = 0
    for p, m in zip(ps, ms):
        u, d, s = classify(p, m, tau, delta)
        with np.errstate(invalid="ignore"):
            then = np.asarray(m) > tau
        new += int(np.count_nonzero(u & ~then))
        changed += int(np.count_nonzero(u & then))
        deleted += int(np.count_nonzero(d))
        suppressed += int(np.count_nonzero(s))
    return {"new": new, "changed": changed, "deleted": deleted, "suppressed": suppressed}


def export(ps, tau):
    """The thresholded state in the (offsets, ids, p) form of group_export_sparse."""
    off = np.zeros(len(ps) + 1, dtype=np.int64)
    ids, vals = [], []
    for i, p in enumerate(ps):
        with np.errstate(invalid="ignore"):
            at = np.nonzero(np.asarray(p) > tau)[0]
        ids.append(at.astype(np.int32))
        vals.append(np.asarray(p, dtype=np.float64)[at])
        off[i + 1] = off[i] + len(at)
    return off, np.concatenate(ids), np.concatenate(vals)


def apply(replica, pt):
    """The replica after the patch, lane by lane with a dict per lane: deletes leave, upserts overwrite or enter, ids ascending."""
    off, ids, p = replica
    n = len(off) - 1
    out_off = np.zeros(n + 1, dtype=np.int64)
    out_ids, out_p = [], []
    for i in range(n):
        lane = {int(v): x for v, x in zip(ids[off[i]:off[i + 1]], p[off[i]:off[i + 1]])}
        for v in pt["del_ids"][pt["del_offsets"][i]:pt["del_offsets"][i + 1]]:
            lane.pop(int(v))  # (a delete of something the replica does not hold is an error of the feed)
        for v, x in zip(pt["up_ids"][pt["up_offsets"][i]:pt["up_offsets"][i + 1]], pt["up_p"][pt["up_offsets"][i]:pt["up_offsets"][i + 1]]):
            lane[int(v)] = x
        keys = sorted(lane)
        out_ids.append(np.array(keys, dtype=np.int32))
        out_p.append(np.array([lane[k] for k in keys], dtype=np.float64))
        out_off[i + 1] = out_off[i] + len(keys)
    return out_off, np.concatenate(out_ids), np.concatenate(out_p)


def remark(ps, ms, tau, delta, mode):
    """The dense marks of every lane after a WRITTEN patch under `mode` (new arrays; ms is left alone)."""
    out = []
    for p, m in zip(ps, ms):
        p, m = np.asarray(p, dtype=np.float64), np.array(m, dtype=np.float64)
        if mode == REMARK_ALL:
            m = p.copy()
        elif mode == REMARK_EMITTED:
            u, d, _ = classify(p, m, tau, delta)
            m[u | d] = p[u | d]
        out.append(m)
    return out


def same_patch(got, want):
    """Offsets and ids exactly, p by bit pattern."""
    return (np.array_equal(got["up_offsets"], want["up_offsets"]) and np.array_equal(got["del_offsets"], want["del_offsets"]) and
            np.array_equal(got["up_ids"], want["up_ids"]) and np.array_equal(got["del_ids"], want["del_ids"]) and
            np.array_equal(bits(got["up_p"]), bits(want["up_p"])))


def same_sparse(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
