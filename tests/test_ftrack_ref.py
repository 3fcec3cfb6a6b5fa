"""The forward track's definition (tests/ftrack_ref.py) on the CPU: a 60-vertex multigraph under a sliding window of 300 edges, 10
deletes and 10 inserts per batch, 20 batches. After every batch the tracked column keeps the entrywise guarantee against the exact
solve, |0.15 (I - M^T)^-1 h - p| <= sum |r| + 1e-12 (the slack of the project's forward tests), and the invariant (I); a fresh track
is tests/fpush_ref.py bit for bit; the fix-up on cases worked by hand. The stream holds a batch in which a tail gains and loses an
edge (d1 == d0), one with a self-loop record, one that removes a vertex's last edge and one that first names a seed that started
rowless. No GPU call is made."""
import numpy as np

from tests import forward_ref as fr
from tests import fpush_ref as pr
from tests import ftrack_ref as tr

V, WN, C, BATCHES = 60, 300, 10, 20
LAST, LATE = 59, 58          # LAST: its only edge leaves in batch 3; LATE: a seed first named by batch 5
SAME_TAIL_BATCH, LOOP_BATCH, LAST_BATCH, LATE_BATCH = 2, 4, 3, 5


def small_stream(seed=3):
    """The stream (tails, heads) of WN + BATCHES * C edges over vertices 0 .. 56, with the four special records placed."""
    rng = np.random.default_rng(seed)
    n = WN + BATCHES * C
    t, h = rng.integers(0, 57, n), rng.integers(0, 57, n)
    t[C * (LAST_BATCH - 1) + 4], h[C * (LAST_BATCH - 1) + 4] = LAST, 7            # deleted by batch 3: LAST's only edge
    t[WN + C * (SAME_TAIL_BATCH - 1) + 2] = t[C * (SAME_TAIL_BATCH - 1) + 6]      # batch 2 inserts at a tail it deletes from
    t[WN + C * (LOOP_BATCH - 1) + 1] = h[WN + C * (LOOP_BATCH - 1) + 1] = 11      # batch 4 inserts 11 -> 11
    t[WN + C * (LATE_BATCH - 1) + 3], h[WN + C * (LATE_BATCH - 1) + 3] = 20, LATE  # batch 5 names LATE for the first time
    return t.astype(np.int64), h.astype(np.int64)


def window(t, h, k):
    return t[C * k:C * k + WN], h[C * k:C * k + WN]


def records(t, h, k):
    """The batch that makes epoch k (k >= 1): C deletes of the oldest edges, then C inserts, as SlidingStream stages a directed one."""
    lo, hi = C * (k - 1), WN + C * (k - 1)
    return (np.concatenate([t[lo:lo + C], t[hi:hi + C]]), np.concatenate([h[lo:lo + C], h[hi:hi + C]]),
            np.concatenate([np.zeros(C, dtype=np.uint8), np.ones(C, dtype=np.uint8)]))


SETS = ((np.array([5]), np.array([1.0])), (np.array([LATE, 12, LAST]), np.array([0.5, 2.0, 0.75])), (np.array([33, 40]), np.array([1.0, 1.0])))


def exact_h(t, h, ids, w):
    return sum(wi * fr.exact(V, t, h, int(q)) for q, wi in zip(ids, w))


def invariant_gap(rows, t, h, col):
    """max |r - (h - P + sum over stored edges 0.85 P[u] / (d(u) + 1))|"""
    P = col.p / fr.ALPHA
    hv = np.zeros(V)
    hv[col.ids] = col.weights
    flow = np.zeros(V)
    np.add.at(flow, h, fr.DAMP * P[t] / (rows.d[t] + 1.0))
    return float(np.max(np.abs(col.r - (hv - P + flow))))


def test_the_special_batches_are_in_the_stream():
    t, h = small_stream()
    w0 = window(t, h, 0)
    assert LATE not in w0[0] and LATE not in w0[1] and np.sum(w0[0] == LAST) + np.sum(w0[1] == LAST) == 1
    bt, bh, ins = records(t, h, SAME_TAIL_BATCH)
    d0, d1 = np.bincount(window(t, h, SAME_TAIL_BATCH - 1)[0], minlength=V), np.bincount(window(t, h, SAME_TAIL_BATCH)[0], minlength=V)
    both = np.intersect1d(bt[ins == 0], bt[ins == 1])
    assert any(d0[u] == d1[u] for u in both)
    bt, bh, ins = records(t, h, LOOP_BATCH)
    assert np.any((bt == bh) & (ins == 1))
    wl = window(t, h, LAST_BATCH)
    assert LAST not in wl[0] and LAST not in wl[1]
    bt, bh, ins = records(t, h, LATE_BATCH)
    assert LATE in bh[ins == 1] and all(LATE not in np.concatenate(window(t, h, k)) for k in range(LATE_BATCH))


def test_a_fresh_track_is_the_forward_push_bit_for_bit():
    t, h = small_stream()
    rows = fr.Rows.from_edges(V, *window(t, h, 0))
    rowless = pr.rowless_mask(rows)
    assert rowless[LATE]
    for ids, w in SETS:
        for eps, cap in ((1e-3, 64), (1e-6, 64), (1e-6, 3)):
            a, b = tr.Column(rows, ids, w, eps, cap), pr.push(rows, rowless, ids, w, eps, cap)
            assert a.p.tobytes() == b.p.tobytes() and a.r.tobytes() == b.r.tobytes()
            assert (a.last.rounds_used, a.last.converged, a.last.pushes, a.last.left) == (b.rounds_used, b.converged, b.pushes, b.left)
            assert np.float64(a.last.rem).tobytes() == np.float64(b.rem).tobytes() and a.last.fix == [0, 0, 0]
            assert tr.work(rows, [a.last]).tolist() == pr.work(rows, [b]).tolist()


def test_the_guarantee_and_the_invariant_after_each_of_20_batches():
    t, h = small_stream()
    rows = fr.Rows.from_edges(V, *window(t, h, 0))
    eps = 1e-6
    cols = [tr.Column(rows, ids, w, eps, 256) for ids, w in SETS]
    negative = tracked = fresh = 0
    for k in range(1, BATCHES + 1):
        wt, wh = window(t, h, k)
        rows = fr.Rows.from_edges(V, wt, wh)
        rec = records(t, h, k)
        for col in cols:
            before = (col.p.copy(), col.r.copy())
            last = col.update(rows, rec, 256)
            assert last.converged == 1 and last.left == 0 and last.fix[0] == 2 * C
            assert np.all(np.abs(col.r) <= eps * (rows.d + 1.0))
            gap = np.abs(exact_h(wt, wh, col.ids, col.weights) - col.p)
            assert np.all(gap <= np.sum(np.abs(col.r)) + 1e-12), (k, gap.max(), np.sum(np.abs(col.r)))
            assert invariant_gap(rows, wt, wh, col) < 1e-14, k
            assert last.rem == float(np.sum(np.abs(col.r))) or abs(last.rem - np.sum(np.abs(col.r))) < 1e-18
            tracked += last.pushes
            fresh += tr.Column(rows, col.ids, col.weights, eps, 256).last.pushes
            if k == LAST_BATCH and LAST in col.ids:   # the vertex without an edge keeps its values
                assert col.p[LAST] != 0.0 and rows.d[LAST] == 0 and np.diff(rows.ptr)[LAST] == 0
            if k < LATE_BATCH and LATE in col.ids:    # still rowless: settled, untouched
                assert col.p[LATE] == 0.15 * 0.5 and col.r[LATE] == 0.0 and before[0][LATE] == col.p[LATE]
        negative += int(any(np.any(tr.fixup(c.p, c.r, rows.d, *rec)[1] < 0) for c in cols))
    assert negative > 0            # a fix-up leaves negative residuals: the signed test is exercised
    assert tracked < fresh         # the tracked state pushes less than a fresh push per epoch
    print("pushes per batch: tracked", tracked / BATCHES / len(SETS), "fresh", fresh / BATCHES / len(SETS))


def test_more_rounds_on_the_own_epoch_reach_the_bits_of_one_call():
    t, h = small_stream()
    rows0, rows1 = fr.Rows.from_edges(V, *window(t, h, 0)), fr.Rows.from_edges(V, *window(t, h, 1))
    ids, w = SETS[1]
    one = tr.Column(rows0, ids, w, 1e-7, 256)
    one.update(rows1, records(t, h, 1), 256)
    step = tr.Column(rows0, ids, w, 1e-7, 256)
    step.update(rows1, records(t, h, 1), 1)
    calls = 1
    assert step.last.converged == 0 and step.last.rounds_used == 1
    while not step.last.converged:
        step.update(rows1, None, 1)
        assert step.last.fix == [0, 0, 0]
        calls += 1
    assert calls == one.last.rounds_used > 2 and step.last.rounds_used == 1   # (the frontier is evaluated once more after a call's last round)
    assert step.p.tobytes() == one.p.tobytes() and step.r.tobytes() == one.r.tobytes()


def test_the_fix_up_by_hand():
    """0 -> 1, 0 -> 2, 1 -> 2 becomes 0 -> 1, 1 -> 2, 1 -> 1, 3 -> 2: the figures of tests/native/ftrack_plan_test.cpp."""
    p, r = np.array([0.3, 0.06, 0.0, 0.0]), np.array([0.0, 0.25, 0.5, 0.0])
    p1, r1 = tr.fixup(p, r, np.array([1.0, 2.0, 0.0, 1.0]), [0, 1, 3], [2, 1, 2], [0, 1, 1])
    g0, g1 = 0.3 / (0.15 * 3.0), 0.06 / (0.15 * 2.0)
    assert p1.tolist() == [(0.3 * 2.0) / 3.0, (0.06 * 3.0) / 2.0, 0.0, 0.0]
    assert r1.tolist() == [0.0 - (-1.0) * g0, (0.25 - g1) + 0.85 * g1, (0.5 - 0.85 * g0) + 0.0, 0.0]
    assert p.tolist() == [0.3, 0.06, 0.0, 0.0]   # the arguments are left alone
    # an insert and a delete at one tail: its p and r keep their bits
    p2, r2 = tr.fixup(np.array([0.123, 0.0]), np.array([0.017, 0.0]), np.array([3.0, 0.0]), [0, 0], [1, 1], [1, 0])
    c = 0.85 * (0.123 / (0.15 * 4.0))
    assert p2[0] == 0.123 and r2[0] == 0.017 and r2[1] == (0.0 + c) - c and not np.signbit(r2[1])
