"""What a batch moved (dppr_mark / dppr_changes and their group forms) against numpy over the dense reads: p_mark from read /
group_read at mark time, p_now from the same at query time, d = p_now - p_mark (one subtraction), `abs(d) > min_delta` as the
filter, np.lexsort((ids, -abs(d))) as the order. Ids are compared with array_equal, delta and p by their bit patterns, moved
with the count before trimming."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_renumbering_gpu import churn_stream
from tests.util import small_stream

pytestmark = pytest.mark.gpu

KS = (1, 10, 1000, 8192)
EPS = 1e-9
MIN_DELTAS = (0.0, 1e-12, 1e-6)
WIDTHS = (1, 2, 3, 8, 9, 10, 16)  # narrow and wide rows, the padding lane, the 8 -> 9 switch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def expected(p_now, p_mark, k, min_delta):
    d = p_now - p_mark
    ids = np.nonzero(np.abs(d) > min_delta)[0]
    moved = len(ids)
    ids = ids[np.lexsort((ids, -np.abs(d[ids])))[:k]]
    return ids.astype(np.int32), d[ids], p_now[ids], moved


def assert_same(got, p_now, p_mark, k, min_delta, what):
    gi, gd, gp, gm = got
    wi, wd, wp, wm = expected(p_now, p_mark, k, min_delta)
    assert np.array_equal(gi, wi), (what, k, min_delta, gi[:8], wi[:8], len(gi), len(wi))
    assert np.array_equal(bits(gd), bits(wd)), (what, k, min_delta)
    assert np.array_equal(bits(gp), bits(wp)), (what, k, min_delta)
    assert gm == wm, (what, k, min_delta, gm, wm)
    return wi, wd


def dense_slot(e, slot):
    return [e.read(slot)[0]]


def dense_group(e, gid, n):
    return [e.group_read(gid, i)[0] for i in range(n)]


def check(e, handle, n, marks, nows, ks=KS, min_deltas=MIN_DELTAS, remark=False, what=""):
    """handle: ("slot", slot) or ("group", gid); marks / nows: the dense columns. Returns every reference seen: (k, ids, d)."""
    seen = []
    for k in ks:
        for md in min_deltas:
            res = [e.changes(handle[1], k, md, remark)] if handle[0] == "slot" else e.group_changes(handle[1], k, md, remark)
            assert len(res) == n
            for i in range(n):
                seen.append((k,) + assert_same(res[i], nows[i], marks[i], k, md, f"{what} {handle[0]} n={n} source {i}"))
    return seen


class Marked:
    """An engine over the small stream with one slot and one group per width, solved and marked; the dense reads at mark time."""

    def __init__(self, directed, widths=WIDTHS, W=600, c=20):
        V, e1, e2 = small_stream()
        self.V, self.W = V, W
        self.srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 16)]
        self.seen_at_mark = np.zeros(V, dtype=bool)
        self.seen_at_mark[e1[:W]] = self.seen_at_mark[e2[:W]] = self.seen_at_mark[self.srcs] = True
        self.g = orc.Graph(V, e1, e2, directed, W, c)
        self.e = eng.Engine(V, W, directed, c)
        self.e.load_window(*self.g.window_edges())
        self.slot = self.e.add_source(self.srcs[0])
        self.groups = {n: self.e.add_source_group(self.srcs[:n]) for n in widths}
        self.e.init_solve(self.slot, EPS)
        for gid in self.groups.values():
            self.e.group_init_solve(gid, EPS)
        self.mark()

    def handles(self):
        return [(("slot", self.slot), 1)] + [(("group", gid), n) for n, gid in self.groups.items()]

    def dense(self):
        return {h: dense_slot(self.e, h[1]) if h[0] == "slot" else dense_group(self.e, h[1], n) for h, n in self.handles()}

    def mark(self):
        self.e.mark(self.slot)
        for gid in self.groups.values():
            self.e.group_mark(gid)
        self.marks = self.dense()

    def update(self, batches):
        for _ in range(batches):
            assert not self.g.stream_updates()
            self.g.inc_construct(1)
            self.e.set_batch(*self.g.batch())
            self.e.slide(*self.g.new_stream())
            self.e.update(self.slot, EPS)
            for gid in self.groups.values():
                self.e.group_update(gid, EPS)


@pytest.mark.parametrize("directed", [1, 0])
def test_every_row_width(directed):
    s = Marked(directed)
    fresh = {h: False for h, _ in s.handles()}
    for batches in (1, 2):  # queried after 1 and after 3 updates, against the mark taken after the init solve
        s.update(batches)
        nows = s.dense()
        for h, n in s.handles():
            seen = check(s.e, h, n, s.marks[h], nows[h], what=f"after {batches}")
            ids = np.concatenate([i for _, i, _ in seen])
            d = np.concatenate([x for _, _, x in seen])
            assert np.any(d > 0) and np.any(d < 0), (h, n)  # the reference itself shows both signs
            new = ids[~s.seen_at_mark[ids]]  # vertices first seen after the mark: their mark is 0
            assert all(np.all(col[new] == 0.0) for col in s.marks[h])
            fresh[h] = fresh[h] or len(new) > 0
            assert any(len(i) < k for k, i, _ in seen) and any(len(i) == k for k, i, _ in seen)  # fewer moved than k = 8192, more than k = 1
    assert all(fresh.values()), fresh
    s.e.close()


def test_no_change_right_after_a_mark():
    s = Marked(1, widths=(1, 3, 10))
    s.update(1)
    s.mark()
    for h, n in s.handles():
        res = [s.e.changes(h[1], 100)] if h[0] == "slot" else s.e.group_changes(h[1], 100)
        assert len(res) == n
        for ids, d, p, moved in res:
            assert len(ids) == 0 and len(d) == 0 and len(p) == 0 and moved == 0
    s.e.close()


def test_remark_is_the_per_batch_feed():
    s = Marked(0, widths=(1, 3, 10))
    s.update(1)
    at_remark = s.dense()
    for h, n in s.handles():
        check(s.e, h, n, s.marks[h], at_remark[h], ks=(1000,), min_deltas=(0.0,), remark=True, what="first feed")
        res = [s.e.changes(h[1], 1000)] if h[0] == "slot" else s.e.group_changes(h[1], 1000)
        assert all(len(ids) == 0 and moved == 0 for ids, _, _, moved in res), h  # the mark is the current p now
    s.update(1)
    nows = s.dense()
    for h, n in s.handles():
        seen = check(s.e, h, n, at_remark[h], nows[h], ks=(10, 8192), min_deltas=(0.0, 1e-12), what="second feed")
        assert any(len(i) for _, i, _ in seen)
    s.e.close()


def star_slot(L, V):
    """A star of L leaves that enter the stream in a shuffled order: L + 1 occupied rows, one slot."""
    rng = np.random.default_rng(3)
    leaves = (rng.permutation(V - 1)[:L] + 1).astype(np.int32)
    assert not np.all(np.diff(leaves) > 0)
    e = eng.Engine(V, L, 0, 1, schedule=eng.SCHEDULE_SYNC)
    e.load_window(np.zeros(L, dtype=np.int32), leaves)
    slot = e.add_source(0)
    sp = e.id_space()
    assert sp["ids"] + sp["parked"] == L + 1
    return e, slot, np.concatenate([[0], leaves]).astype(np.int64)


@pytest.mark.parametrize("rows", [127, 128, 129, 511, 512, 513, 4097])
def test_crafted_states_at_the_tile_and_chunk_edges(rows):
    """States set by dppr_write at the window's vertices only: `rows` occupied rows around the 128 rows of a tile of the delta
    kernel, the 512 rows of a chunk of the selection's streaming passes and 8 such chunks. Exact ties of |d| with opposite and
    with equal signs (the id order decides); every |d| inside one binade (the candidate list holds every row and all
    refinement rounds run); more qualifiers than k, and fewer."""
    V = 8192
    e, slot, touched = star_slot(rows - 1, V)
    rng = np.random.default_rng(rows)
    zeros = np.zeros(V)
    ks = (1, 10, rows - 1, rows, min(rows + 1, 8192), 8192)

    def crafted(base, delta, min_deltas, what):
        p = np.zeros(V)
        p[touched] = base
        e.write(slot, p, zeros)
        e.mark(slot)
        mark = dense_slot(e, slot)
        assert np.array_equal(bits(mark[0]), bits(p))
        q = p.copy()
        q[touched] += delta
        e.write(slot, q, zeros)
        now = dense_slot(e, slot)  # (the reference comes from the read, not from the arrays passed in)
        sp = e.id_space()
        assert sp["ids"] + sp["parked"] == rows
        return now[0] - mark[0], check(e, ("slot", slot), 1, mark, now, ks=ks, min_deltas=min_deltas, what=what)

    # ties: +1/8, -1/8 and +1/4 in turn, all exact (p = 1/2 everywhere at the mark)
    delta = np.choose(np.arange(rows) % 3, [0.125, -0.125, 0.25])
    d, seen = crafted(0.5, delta, (0.0, 0.125, 0.2), "ties")
    assert set(np.unique(np.abs(d[touched]))) == {0.125, 0.25} and np.any(d == 0.125) and np.any(d == -0.125)
    assert any(len(i) == rows - 1 and np.any(x == 0.125) and np.any(x == -0.125) for _, i, x in seen)  # k = rows - 1 cuts the tie of both signs
    # one binade: |d| in [1, 2) with either sign, a block of equal values among them; some vertices do not move at all
    mag = 1.0 + rng.integers(0, 1 << 20, rows) / float(1 << 20)
    mag[: rows // 4] = mag[0]
    delta = mag * rng.choice([-1.0, 1.0], rows)
    still = rng.permutation(rows)[: rows // 8]
    delta[still] = 0.0
    d, seen = crafted(4.0, delta, (0.0, 1.5), "one binade")
    moved = np.abs(d[touched])
    assert np.all((moved[moved > 0] >= 1.0) & (moved[moved > 0] < 2.0)) and np.count_nonzero(moved) == rows - len(still)
    lengths = [len(i) for _, i, _ in seen]
    assert min(lengths) == 1 and max(lengths) == rows - len(still)  # fewer than k, and more than k
    e.close()


def test_renumbering_between_mark_and_query():
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    sources = list(range(10))
    slot = e.add_source(0)
    gid = e.add_source_group(sources)
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    e.mark(slot)
    e.group_mark(gid)
    at_mark = e.id_space()
    m_slot, m_group = dense_slot(e, slot), dense_group(e, gid, 10)
    parked_between = 0
    for _ in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.update(slot, EPS)
        e.group_update(gid, EPS)
        parked_between = max(parked_between, e.id_space()["parked"])
    sp = e.id_space()
    assert sp["renumberings"] > at_mark["renumberings"], (at_mark, sp)  # the ids were renumbered between mark and query
    assert parked_between > 0 and sp["parked"] > 0, sp
    check(e, ("slot", slot), 1, m_slot, dense_slot(e, slot), ks=(10, 1000, 8192), min_deltas=(0.0, 1e-6), what="renumbered")
    check(e, ("group", gid), 10, m_group, dense_group(e, gid, 10), ks=(10, 8192), min_deltas=(0.0, 1e-6), what="renumbered")
    e.close()


def test_a_change_of_the_sources_drops_the_mark():
    s = Marked(1, widths=(3,))
    gid = s.groups[3]
    churn = [lambda: s.e.group_replace_source(gid, 1, s.srcs[5]), lambda: s.e.group_add_source(gid, s.srcs[6]),
             lambda: s.e.group_remove_source(gid, 0)]
    for change, n in zip(churn, (3, 4, 3)):
        change()
        with pytest.raises(eng.DpprError):
            s.e.group_changes(gid, 10)
        s.groups = {n: gid}
        s.mark()
        s.update(1)
        h = ("group", gid)
        seen = check(s.e, h, n, s.marks[h], s.dense()[h], ks=(10, 8192), min_deltas=(0.0, 1e-12), what="after a change of the sources")
        assert any(len(i) for _, i, _ in seen)
    s.e.close()


def test_invalid_arguments_are_rejected_and_nothing_is_written():
    s = Marked(1, widths=(2,))
    s.update(1)
    e, gid, slot = s.e, s.groups[2], s.slot
    unmarked = e.add_source_group(s.srcs[:2])
    e.unmark(slot)
    e.unmark(slot)  # unmarking something unmarked is fine
    L, h = eng.lib(), e._h
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    K = 16
    ids = np.full(3 * K, 77, dtype=np.int32)
    d = np.full(3 * K, 3.25)
    p = np.full(3 * K, 4.5)
    cnt = np.full(3, 99, dtype=np.int32)
    moved = np.full(3, 55, dtype=np.int32)
    I, D, P, N, M = ids.ctypes.data_as(ip), d.ctypes.data_as(dp), p.ctypes.data_as(dp), cnt.ctypes.data_as(ip), moved.ctypes.data_as(ip)

    def untouched():
        return np.all(ids == 77) and np.all(d == 3.25) and np.all(p == 4.5) and np.all(cnt == 99) and np.all(moved == 55)

    bad = [(unmarked, K, 0.0, 0, I, D, P, N, M),  # no mark
           (gid, 0, 0.0, 0, I, D, P, N, M), (gid, 8193, 0.0, 0, I, D, P, N, M), (gid, -1, 0.0, 0, I, D, P, N, M),
           (gid, K, -1.0, 0, I, D, P, N, M), (gid, K, -1e-300, 1, I, D, P, N, M), (gid, K, float("nan"), 0, I, D, P, N, M),
           (gid, K, 0.0, 0, None, D, P, N, M), (gid, K, 0.0, 0, I, None, P, N, M), (gid, K, 0.0, 0, I, D, P, None, M),
           (7, K, 0.0, 0, I, D, P, N, M), (-1, K, 0.0, 0, I, D, P, N, M)]
    for a in bad:
        assert L.dppr_group_changes(h, *a) == -1, a
        assert untouched(), a
    bad_slot = [(slot, K, 0.0, 0, I, D, P, N, M),  # no mark (unmarked above)
                (3, K, 0.0, 0, I, D, P, N, M), (-1, K, 0.0, 0, I, D, P, N, M)]
    for a in bad_slot:
        assert L.dppr_changes(h, *a) == -1, a
        assert untouched(), a
    e.mark(slot)
    for a in [(slot, 0, 0.0, 0, I, D, P, N, M), (slot, 8193, 0.0, 0, I, D, P, N, M), (slot, K, -1.0, 0, I, D, P, N, M),
              (slot, K, float("nan"), 0, I, D, P, N, M)]:
        assert L.dppr_changes(h, *a) == -1, a
        assert untouched(), a
    for fn in (L.dppr_mark, L.dppr_unmark):
        assert fn(h, 3) == -1 and fn(h, -1) == -1
    for fn in (L.dppr_group_mark, L.dppr_group_unmark):
        assert fn(h, 7) == -1 and fn(h, -1) == -1
    # the rejected calls left the group's mark alone; NULL out_p / out_moved are allowed; a valid call writes exactly [n][k]
    assert L.dppr_group_changes(h, gid, K, 0.0, 0, I, D, None, N, None) == 0
    assert np.all(p == 4.5) and np.all(moved == 55) and np.all(ids[2 * K:] == 77) and np.all(d[2 * K:] == 3.25) and cnt[2] == 99
    nows = dense_group(e, gid, 2)
    for i in range(2):
        wi, wd, _, _ = expected(nows[i], s.marks[("group", gid)][i], K, 0.0)
        assert cnt[i] == len(wi) == K and np.array_equal(ids[i * K:(i + 1) * K], wi) and np.array_equal(bits(d[i * K:(i + 1) * K]), bits(wd))
    assert L.dppr_group_changes(h, gid, K, 1e300, 0, I, D, P, N, M) == 0  # nothing qualifies: counts 0, then -1 / 0.0
    assert np.all(cnt[:2] == 0) and np.all(moved[:2] == 0) and cnt[2] == 99 and moved[2] == 55
    assert np.all(ids[:2 * K] == -1) and np.all(d[:2 * K] == 0.0) and np.all(p[:2 * K] == 0.0)
    assert np.all(ids[2 * K:] == 77) and np.all(d[2 * K:] == 3.25) and np.all(p[2 * K:] == 4.5)
    e.close()


def test_the_topk_queries_are_untouched():
    s = Marked(1, widths=(3, 10))
    s.update(1)
    w = np.random.default_rng(4).standard_normal((4, 10))

    def snapshot():
        out = [s.e.topk(s.slot, k, mp) for k in (10, 8192) for mp in (0.0, 1e-4)]
        out += [x for k in (10, 8192) for gid in s.groups.values() for x in s.e.group_topk(gid, k)]
        out += [x for k in (10, 8192) for x in s.e.group_topk_weighted(s.groups[10], w, k)]
        return out

    before = snapshot()
    for remark in (False, True):
        assert s.e.changes(s.slot, 8192, 0.0, remark)[3] > 0
        for gid in s.groups.values():
            s.e.group_changes(gid, 8192, 0.0, remark)
        after = snapshot()
        assert len(after) == len(before)
        for a, b in zip(after, before):
            assert len(a) == len(b)
            assert np.array_equal(a[0], b[0]) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[1:], b[1:]))
    s.e.close()


def test_marks_and_scratch_go_with_unmark_and_with_the_engine():
    gc.collect()
    before = eng.live_bytes()
    s = Marked(1, widths=(10,))
    gid = s.groups[10]
    s.update(1)
    held = eng.live_bytes()
    res = s.e.group_changes(gid, 8192)
    assert len(res) == 10 and any(len(ids) for ids, _, _, _ in res)
    s.e.changes(s.slot, 8192)
    with_scratch = eng.live_bytes()
    assert with_scratch[0] > held[0] and with_scratch[1] > held[1]  # (the scratch states and the result blocks are there)
    s.e.group_unmark(gid)
    assert eng.live_bytes()[0] == with_scratch[0] - 8 * s.V * 10  # rows of 10 doubles
    s.e.unmark(s.slot)
    assert eng.live_bytes()[0] == with_scratch[0] - 8 * s.V * 11
    s.e.group_unmark(gid)  # (nothing left to release)
    assert eng.live_bytes()[0] == with_scratch[0] - 8 * s.V * 11
    with pytest.raises(eng.DpprError):
        s.e.group_changes(gid, 10)
    s.e.group_mark(gid)  # a mark that goes with the engine
    s.e.close()
    gc.collect()
    assert eng.live_bytes() == before
