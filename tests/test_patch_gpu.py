"""The patch feed (dppr_patch / dppr_group_patch) against the numpy restatement of tests/patch_ref.py over the dense reads: p_mark
from read / group_read at mark time, p_now from the same at query time. Offsets and ids are compared with array_equal, p by its
bit pattern, for host and device destinations; the effect of a re-mark is read back through group_changes(k = 8192, min_delta = 0)
against the reference's dense mark."""
import ctypes as C

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests import patch_ref as ref
from tests.test_changes_gpu import EPS, Marked, dense_group, dense_slot, expected as changes_expected, star_slot
from tests.test_export_gpu import Hip
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

# 0, 1e-12 and 1e-6, and 1e-3 beside them: on the oracle's states of this stream no entry that stays in the support of a one- or
# two-lane handle moves by 1e-6 or less in three batches (3 lanes: 2 entries), whatever the threshold, so only the coarser delta
# shows the suppressed kind on every handle (hundreds of entries)
DELTAS = (0.0, 1e-12, 1e-6, 1e-3)
# of the marked positive p of a handle: on the oracle's states every handle, directed or not, shows entries entering (>= 264),
# changing (>= 1885) and leaving (>= 48) across these thresholds within three batches
QUANTILES = (0.5, 0.9)
KEEP, ALL, EMITTED = eng.PATCH_KEEP_MARK, eng.PATCH_REMARK_ALL, eng.PATCH_REMARK_EMITTED
I64P = C.POINTER(C.c_int64)


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def host_patch(e, h, tau, delta, remark=KEEP):
    return e.patch(h[1], tau, delta, remark) if h[0] == "slot" else e.group_patch(h[1], tau, delta, remark)


class DevDest:
    """Device arrays of the caller, obtained once (an allocation waits for the whole device): n * V entries of every kind."""

    def __init__(self, hip, entries):
        self.hip, self.entries = hip, entries
        self.up_ids, self.up_p, self.del_ids = hip.alloc(4 * entries), hip.alloc(8 * entries), hip.alloc(4 * entries)

    def call(self, e, h, tau, delta, cap_up, cap_del, remark=KEEP):
        fn = e.patch_dev if h[0] == "slot" else e.group_patch_dev
        return fn(h[1], tau, delta, cap_up, cap_del, self.up_ids, self.up_p, self.del_ids, remark)

    def patch(self, e, h, n, tau, delta, remark=KEEP):
        """The size call, then the fill with exact caps."""
        uo, do, written = self.call(e, h, tau, delta, 0, 0)
        ups, dels = int(uo[n]), int(do[n])
        assert written == (1 if ups == 0 and dels == 0 else 0)
        uo2, do2, written = self.call(e, h, tau, delta, ups, dels, remark)
        assert written == 1 and np.array_equal(uo, uo2) and np.array_equal(do, do2)
        return {"up_offsets": uo, "up_ids": self.hip.read(self.up_ids, 4 * ups, np.int32), "up_p": self.hip.read(self.up_p, 8 * ups, np.float64),
                "del_offsets": do, "del_ids": self.hip.read(self.del_ids, 4 * dels, np.int32)}

    def untouched(self):
        return all(np.all(self.hip.read(ptr, nb) == 0xAB) for ptr, nb in ((self.up_ids, 4 * self.entries), (self.up_p, 8 * self.entries),
                                                                            (self.del_ids, 4 * self.entries)))


def thresholds(marks):
    """0, two quantiles of the handle's marked positive p, and 1.0 (above every p: nothing qualifies)."""
    pos = np.concatenate([m[m > 0] for m in marks])
    return (0.0,) + tuple(float(np.quantile(pos, q)) for q in QUANTILES) + (1.0,)


def all_changes(e, h):
    """Every id of every lane whose p differs from the mark, with its delta (k = 8192 holds them all in these tests)."""
    res = [e.changes(h[1], 8192, 0.0)] if h[0] == "slot" else e.group_changes(h[1], 8192, 0.0)
    assert all(moved == len(ids) for ids, _, _, moved in res)
    return res


def mark_differs_at(e, h):
    """Per lane, the set of ids where the mark on the device differs from p."""
    return [set(int(v) for v in ids) for ids, _, _, _ in all_changes(e, h)]


def assert_mark_is(e, h, n, nows, want, what):
    """The mark on the device against the reference's dense mark, read through the changes query: the same ids differ from p, by
    the same delta, bit for bit."""
    res = all_changes(e, h)
    assert len(res) == n
    for i in range(n):
        wi, wd, _, wm = changes_expected(nows[i], want[i], 8192, 0.0)
        assert wm <= 8192
        assert np.array_equal(res[i][0], wi) and np.array_equal(ref.bits(res[i][1]), ref.bits(wd)), (what, h, i)


@pytest.mark.parametrize("directed", [1, 0])
def test_every_row_width(hip, directed):
    s = Marked(directed)
    dev = DevDest(hip, 16 * s.V)
    taus = {h: thresholds(s.marks[h]) for h, _ in s.handles()}
    shown = {h: {"new": 0, "changed": 0, "deleted": 0, "suppressed": 0} for h, _ in s.handles()}
    for batches in (1, 2):  # patched after 1 and after 3 updates, against the mark taken after the init solve
        s.update(batches)
        nows = s.dense()
        for h, n in s.handles():
            for tau in taus[h]:
                for delta in DELTAS:
                    want = ref.patch(nows[h], s.marks[h], tau, delta)
                    assert ref.same_patch(host_patch(s.e, h, tau, delta), want), (h, n, tau, delta, "host")
                    assert ref.same_patch(dev.patch(s.e, h, n, tau, delta), want), (h, n, tau, delta, "device")
                    for kind, count in ref.kinds(nows[h], s.marks[h], tau, delta).items():
                        shown[h][kind] += count
            assert ref.patch(nows[h], s.marks[h], 1.0, 0.0)["up_offsets"][-1] == 0  # above every p: an empty patch
    for h, kinds in shown.items():  # the reference itself shows all four kinds, for every handle
        assert all(count > 0 for count in kinds.values()), (h, kinds)
    s.e.close()


@pytest.mark.parametrize("delta", [0.0, 1e-7])
def test_the_replica_follows_the_state(delta):
    """apply_patch chained from the initial export, with the emitted-only re-mark: delta = 0 -- the replica IS the export after every
    batch, bit for bit; delta > 0 -- the same support, every value within delta."""
    s = Marked(0, widths=(1, 3, 10))
    replicas = {}

    def export(h, tau):
        return s.e.export_sparse(h[1], tau) if h[0] == "slot" else s.e.group_export_sparse(h[1], tau)

    for h, n in s.handles():
        tau = thresholds(s.marks[h])[1]
        replicas[h] = (tau, export(h, tau))  # the initial sync: the mark (Marked), then the export
    for batch in range(6):
        s.update(1)
        for h, n in s.handles():
            tau, replica = replicas[h]
            before = replica
            pt = host_patch(s.e, h, tau, delta, EMITTED)
            replica = eng.apply_patch(replica, pt)
            want = export(h, tau)
            assert np.array_equal(replica[0], want[0]) and np.array_equal(replica[1], want[1]), (h, batch)
            if delta == 0.0:
                assert np.array_equal(ref.bits(replica[2]), ref.bits(want[2])), (h, batch)
            else:
                assert np.all(np.abs(replica[2] - want[2]) <= delta), (h, batch)
            assert ref.same_sparse(replica, ref.apply(before, pt))
            replicas[h] = (tau, replica)
    s.e.close()


@pytest.mark.parametrize("mode", [KEEP, ALL, EMITTED])
def test_remark_modes(mode):
    s = Marked(1, widths=(1, 3, 10))
    s.update(1)
    nows = s.dense()
    delta = 1e-7
    for h, n in s.handles():
        tau = thresholds(s.marks[h])[1]
        want = ref.patch(nows[h], s.marks[h], tau, delta)
        assert want["up_offsets"][-1] > 0
        assert ref.same_patch(host_patch(s.e, h, tau, delta, mode), want), (h, mode)
        after = ref.remark(nows[h], s.marks[h], tau, delta, mode)
        assert_mark_is(s.e, h, n, nows[h], after, f"mode {mode}")
        again = host_patch(s.e, h, tau, delta)
        assert ref.same_patch(again, ref.patch(nows[h], after, tau, delta)), (h, mode)
        if mode == KEEP:
            assert ref.same_patch(again, want)
        else:
            assert again["up_offsets"][-1] == 0 and again["del_offsets"][-1] == 0  # the second patch is empty
        if mode == ALL:
            assert all(len(ids) == 0 for ids in mark_differs_at(s.e, h))  # the mark is p everywhere
        if mode == EMITTED:  # the mark differs from p exactly at the non-emitted entries that moved
            for i, differs in enumerate(mark_differs_at(s.e, h)):
                u, d, _ = ref.classify(nows[h][i], s.marks[h][i], tau, delta)
                moved = nows[h][i] != s.marks[h][i]
                assert differs == set(int(v) for v in np.nonzero(moved & ~(u | d))[0]) and len(differs) > 0, (h, i)
    s.e.close()


def test_capacity(hip):
    s = Marked(1, widths=(3, 10))
    s.update(1)
    nows = s.dense()
    dev = DevDest(hip, 10 * s.V)
    for h, n in s.handles():
        tau = thresholds(s.marks[h])[1]
        want = ref.patch(nows[h], s.marks[h], tau, 0.0)
        ups, dels = int(want["up_offsets"][-1]), int(want["del_offsets"][-1])
        assert ups > 1 and dels > 0, (h, ups, dels)
        for cap_up, cap_del in ((ups - 1, dels), (ups, dels - 1), (ups - 1, dels - 1), (0, dels), (ups, 0)):
            uo, do, written = dev.call(s.e, h, tau, 0.0, cap_up, cap_del, EMITTED)
            assert written == 0 and np.array_equal(uo, want["up_offsets"]) and np.array_equal(do, want["del_offsets"])  # the offsets are true
            assert dev.untouched(), (h, cap_up, cap_del)
            # host destination: guard values stay
            up_ids, up_p, del_ids = np.full(ups, -77, dtype=np.int32), np.full(ups, 3.25), np.full(dels, -78, dtype=np.int32)
            uo, do = np.full(n + 1, -5, dtype=np.int64), np.full(n + 1, -5, dtype=np.int64)
            out = eng.PatchOut(uo.ctypes.data_as(I64P), up_ids.ctypes.data, up_p.ctypes.data, do.ctypes.data_as(I64P), del_ids.ctypes.data, -1)
            fn = eng.lib().dppr_patch if h[0] == "slot" else eng.lib().dppr_group_patch
            assert fn(s.e._h, h[1], tau, 0.0, cap_up, cap_del, eng.DEST_HOST, EMITTED, C.byref(out)) == 0
            assert out.written == 0 and np.array_equal(uo, want["up_offsets"]) and np.array_equal(do, want["del_offsets"])
            assert np.all(up_ids == -77) and np.all(up_p == 3.25) and np.all(del_ids == -78)
            assert_mark_is(s.e, h, n, nows[h], s.marks[h], "a cap one short")  # the mark is unchanged even with the emitted-only re-mark
        uo, do, written = dev.call(s.e, h, tau, 0.0, ups, dels, EMITTED)  # the same call with exact caps succeeds
        assert written == 1
        got = {"up_offsets": uo, "up_ids": hip.read(dev.up_ids, 4 * ups, np.int32), "up_p": hip.read(dev.up_p, 8 * ups, np.float64),
               "del_offsets": do, "del_ids": hip.read(dev.del_ids, 4 * dels, np.int32)}
        assert ref.same_patch(got, want)
        assert np.all(hip.read(dev.up_ids + 4 * ups, 64) == 0xAB) and np.all(hip.read(dev.del_ids + 4 * dels, 64) == 0xAB)
        assert_mark_is(s.e, h, n, nows[h], ref.remark(nows[h], s.marks[h], tau, 0.0, EMITTED), "exact caps")
        assert hip.L.hipMemset(dev.up_ids, 0xAB, 4 * dev.entries) == 0 and hip.L.hipMemset(dev.up_p, 0xAB, 8 * dev.entries) == 0
        assert hip.L.hipMemset(dev.del_ids, 0xAB, 4 * dev.entries) == 0 and hip.L.hipDeviceSynchronize() == 0
    s.e.close()


@pytest.mark.parametrize("rows", [63, 64, 65, 255, 256, 257, 513])
def test_crafted_slot_at_the_tile_and_wave_edges(hip, rows):
    """A slot over V = 8192 ids set by dppr_write: entries of every kind at the first and last thread of a wave (64 ids) and of a tile
    (256 ids), a tile without an entry between two tiles that have some, tau between neighbouring doubles, and a vertex with a
    qualifying mark whose p is then written to 0.0. The occupied rows are `rows`; every other id has no internal id."""
    V = 8192
    e, slot, touched = star_slot(rows - 1, V)
    h = ("slot", slot)
    tau = 0.25
    above, below = np.nextafter(tau, 1.0), tau  # neighbouring doubles: the first qualifies, the second does not
    delta = 2.0 ** -10
    zeros = np.zeros(V)
    # the ids the window touches are scattered (the exact threads: the next test); the kinds go out in turn along the sorted ids
    ids = np.sort(touched)
    in_quiet_tile = (ids >= 1024) & (ids < 1280)  # the tile [1024, 1280) gets no entry: marks and p equal there
    kinds = np.arange(len(ids)) % 5  # 0 new, 1 changed above delta, 2 suppressed, 3 left, 4 left by a write of 0.0
    mark = np.zeros(V)
    now = np.zeros(V)
    mark[ids] = np.choose(kinds, [below, 0.5, 0.5, above, 0.5])
    now[ids] = np.choose(kinds, [above, 0.5 + 2 * delta, 0.5 + delta, below, 0.0])
    now[ids[in_quiet_tile]] = mark[ids[in_quiet_tile]]
    e.write(slot, mark, zeros)
    e.mark(slot)
    m = dense_slot(e, slot)
    assert np.array_equal(ref.bits(m[0]), ref.bits(mark))
    e.write(slot, now, zeros)
    p = dense_slot(e, slot)  # (the reference comes from the read, not from the arrays passed in)
    dev = DevDest(hip, V)
    for t, d in ((tau, delta), (tau, 0.0), (0.0, delta), (np.nextafter(tau, 0.0), delta)):  # (the last: a p of exactly tau qualifies)
        want = ref.patch(p, m, t, d)
        assert ref.same_patch(host_patch(e, h, t, d), want), (rows, t, d)
        assert ref.same_patch(dev.patch(e, h, 1, t, d), want), (rows, t, d)
    want = ref.patch(p, m, tau, delta)
    shown = ref.kinds(p, m, tau, delta)
    assert all(c > 0 for c in shown.values()), shown
    assert np.any(p[0][want["del_ids"]] == 0.0) and np.any(p[0][want["del_ids"]] > 0.0)  # both ways to leave
    emitted = set(int(v) for v in want["up_ids"]) | set(int(v) for v in want["del_ids"])
    assert not any(1024 <= v < 1280 for v in emitted)
    assert any(v < 1024 for v in emitted) and any(v >= 1280 for v in emitted)
    # the re-marks on the crafted state
    for mode in (EMITTED, ALL):
        e.write(slot, mark, zeros)
        e.mark(slot)
        e.write(slot, now, zeros)
        assert ref.same_patch(host_patch(e, h, tau, delta, mode), want)
        assert_mark_is(e, h, 1, p, ref.remark(p, m, tau, delta, mode), f"crafted, mode {mode}")
    e.close()


def test_entries_at_chosen_threads_of_a_wave_and_a_tile():
    """Every id of [0, 1280) is given an internal id by a path graph, so the kinds can be put at exact threads: the first and the last
    thread of a wave and of a tile hold one entry of each kind in turn, tile 2 ([512, 768)) holds none."""
    V, L = 8192, 1279
    e = eng.Engine(V, L, 0, 1, schedule=eng.SCHEDULE_SYNC)
    e.load_window(np.arange(L, dtype=np.int32), np.arange(1, L + 1, dtype=np.int32))
    slot = e.add_source(0)
    h = ("slot", slot)
    tau, delta = 0.25, 2.0 ** -10
    above = np.nextafter(tau, 1.0)
    mark_of = [tau, 0.5, 0.5, above, 0.5]  # new, changed, suppressed, left, left by a write of 0.0
    now_of = [above, 0.5 + 2 * delta, 0.5 + delta, tau, 0.0]
    mark, now, zeros = np.zeros(V), np.zeros(V), np.zeros(V)
    spots = [v for t in (0, 256, 768, 1024) for v in (t, t + 1, t + 62, t + 63, t + 64, t + 65, t + 126, t + 127, t + 128, t + 191, t + 192, t + 254, t + 255)]
    for j, v in enumerate(spots):
        mark[v], now[v] = mark_of[j % 5], now_of[j % 5]
    mark[512:768] = now[512:768] = 0.5  # the tile between: in the support, unmoved
    e.write(slot, mark, zeros)
    e.mark(slot)
    m = dense_slot(e, slot)
    e.write(slot, now, zeros)
    p = dense_slot(e, slot)
    assert np.array_equal(ref.bits(m[0]), ref.bits(mark)) and np.array_equal(ref.bits(p[0]), ref.bits(now))
    want = ref.patch(p, m, tau, delta)
    assert sorted(want["up_ids"].tolist() + want["del_ids"].tolist()) == sorted(v for j, v in enumerate(spots) if j % 5 != 2)
    assert ref.same_patch(host_patch(e, h, tau, delta), want)
    assert ref.same_patch(host_patch(e, h, tau, delta, EMITTED), want)
    assert_mark_is(e, h, 1, p, ref.remark(p, m, tau, delta, EMITTED), "chosen threads")
    e.close()


def test_renumbering_and_parking_between_mark_and_patch():
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    slot = e.add_source(0)
    gid = e.add_source_group(list(range(10)))
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
    assert sp["renumberings"] > at_mark["renumberings"], (at_mark, sp)  # the ids were renumbered between mark and patch
    assert parked_between > 0 and sp["parked"] > 0, sp
    for h, n, marks, nows in ((("slot", slot), 1, m_slot, dense_slot(e, slot)), (("group", gid), 10, m_group, dense_group(e, gid, 10))):
        for tau in thresholds(marks)[:3]:
            for delta in (0.0, 1e-6):
                want = ref.patch(nows, marks, tau, delta)
                assert want["up_offsets"][-1] > 0 and (tau == 0.0 or want["del_offsets"][-1] > 0)
                assert ref.same_patch(host_patch(e, h, tau, delta), want), (h, tau, delta)
        tau = thresholds(marks)[1]
        assert ref.same_patch(host_patch(e, h, tau, 1e-6, EMITTED), ref.patch(nows, marks, tau, 1e-6))
        assert_mark_is(e, h, n, nows, ref.remark(nows, marks, tau, 1e-6, EMITTED), "renumbered")
    e.close()


def test_a_churn_call_drops_the_mark():
    s = Marked(1, widths=(3,))
    s.update(1)
    gid = s.groups[3]
    s.e.group_replace_source(gid, 1, s.srcs[5])
    uo, do = np.full(4, -5, dtype=np.int64), np.full(4, -6, dtype=np.int64)
    ids, p, dl = np.full(8, -77, dtype=np.int32), np.full(8, 3.25), np.full(8, -78, dtype=np.int32)
    out = eng.PatchOut(uo.ctypes.data_as(I64P), ids.ctypes.data, p.ctypes.data, do.ctypes.data_as(I64P), dl.ctypes.data, 55)
    assert eng.lib().dppr_group_patch(s.e._h, gid, 0.0, 0.0, 8, 8, eng.DEST_HOST, EMITTED, C.byref(out)) == -1
    assert np.all(uo == -5) and np.all(do == -6) and np.all(ids == -77) and np.all(p == 3.25) and np.all(dl == -78) and out.written == 55
    with pytest.raises(eng.DpprError):
        s.e.group_patch(gid, 0.0)
    s.groups = {3: gid}
    s.mark()  # the consumer marks and exports again
    s.update(1)
    h = ("group", gid)
    want = ref.patch(s.dense()[h], s.marks[h], 0.0, 0.0)
    assert want["up_offsets"][-1] > 0 and ref.same_patch(host_patch(s.e, h, 0.0, 0.0), want)
    s.e.close()


def test_invalid_arguments_are_rejected_and_nothing_is_written(hip):
    s = Marked(1, widths=(2,))
    s.update(1)
    e, gid, slot = s.e, s.groups[2], s.slot
    h = ("group", gid)
    nows = s.dense()[h]
    unmarked = e.add_source_group(s.srcs[:2])
    L = eng.lib()
    cap = 2 * s.V
    uo, do = np.full(3, -5, dtype=np.int64), np.full(3, -6, dtype=np.int64)
    ids, p, dl = np.full(cap, -77, dtype=np.int32), np.full(cap, 3.25), np.full(cap, -78, dtype=np.int32)
    UO, DO, I, P, D = uo.ctypes.data_as(I64P), do.ctypes.data_as(I64P), ids.ctypes.data, p.ctypes.data, dl.ctypes.data
    d_ids, d_p, d_del = hip.alloc(4 * cap), hip.alloc(8 * cap), hip.alloc(4 * cap)
    short_ids, short_p, short_del = hip.alloc(4 * cap - 4), hip.alloc(8 * cap - 8), hip.alloc(4 * cap - 4)
    nan = float("nan")

    def untouched():
        host = np.all(uo == -5) and np.all(do == -6) and np.all(ids == -77) and np.all(p == 3.25) and np.all(dl == -78)
        dev = all(np.all(hip.read(ptr, nb) == 0xAB) for ptr, nb in ((d_ids, 4 * cap), (d_p, 8 * cap), (d_del, 4 * cap), (short_ids, 4 * cap - 4),
                                                                    (short_p, 8 * cap - 8), (short_del, 4 * cap - 4)))
        return host and dev

    H, Dv = eng.DEST_HOST, eng.DEST_DEVICE
    # (handle, tau, delta, cap_up, cap_del, dest, remark, the out block)
    bad = [(unmarked, 0.0, 0.0, cap, cap, H, EMITTED, (UO, I, P, DO, D)),  # no mark
           (gid, -1.0, 0.0, cap, cap, H, EMITTED, (UO, I, P, DO, D)), (gid, -1e-300, 0.0, cap, cap, H, ALL, (UO, I, P, DO, D)),
           (gid, nan, 0.0, cap, cap, H, EMITTED, (UO, I, P, DO, D)), (gid, 0.0, -1.0, cap, cap, H, EMITTED, (UO, I, P, DO, D)),
           (gid, 0.0, nan, cap, cap, H, ALL, (UO, I, P, DO, D)), (gid, 0.0, 0.0, -1, cap, H, EMITTED, (UO, I, P, DO, D)),
           (gid, 0.0, 0.0, cap, -1, H, EMITTED, (UO, I, P, DO, D)), (gid, 0.0, 0.0, cap, cap, 2, EMITTED, (UO, I, P, DO, D)),
           (gid, 0.0, 0.0, cap, cap, -1, EMITTED, (UO, I, P, DO, D)), (gid, 0.0, 0.0, cap, cap, H, 3, (UO, I, P, DO, D)),
           (gid, 0.0, 0.0, cap, cap, H, -1, (UO, I, P, DO, D)), (gid, 0.0, 0.0, cap, cap, H, EMITTED, (None, I, P, DO, D)),
           (gid, 0.0, 0.0, cap, cap, H, EMITTED, (UO, I, P, None, D)), (gid, 0.0, 0.0, cap, cap, H, EMITTED, (UO, None, P, DO, D)),
           (gid, 0.0, 0.0, cap, cap, H, EMITTED, (UO, I, None, DO, D)), (gid, 0.0, 0.0, cap, cap, H, EMITTED, (UO, I, P, DO, None)),
           (7, 0.0, 0.0, cap, cap, H, EMITTED, (UO, I, P, DO, D)), (-1, 0.0, 0.0, cap, cap, H, EMITTED, (UO, I, P, DO, D)),
           # device pointers that are host memory, or short by one entry
           (gid, 0.0, 0.0, cap, cap, Dv, EMITTED, (UO, I, d_p, DO, d_del)), (gid, 0.0, 0.0, cap, cap, Dv, EMITTED, (UO, d_ids, P, DO, d_del)),
           (gid, 0.0, 0.0, cap, cap, Dv, EMITTED, (UO, d_ids, d_p, DO, D)), (gid, 0.0, 0.0, cap, cap, Dv, ALL, (UO, short_ids, d_p, DO, d_del)),
           (gid, 0.0, 0.0, cap, cap, Dv, ALL, (UO, d_ids, short_p, DO, d_del)), (gid, 0.0, 0.0, cap, cap, Dv, ALL, (UO, d_ids, d_p, DO, short_del)),
           (gid, 0.0, 0.0, cap, cap, Dv, ALL, (UO, d_ids + 2, d_p, DO, d_del)), (gid, 0.0, 0.0, cap, cap, Dv, ALL, (UO, d_ids, d_p + 4, DO, d_del))]
    for a in bad:
        out = eng.PatchOut(a[7][0], a[7][1], a[7][2], a[7][3], a[7][4], 55)
        assert L.dppr_group_patch(e._h, *a[:7], C.byref(out)) == -1, a
        assert out.written == 55 and untouched(), a
    assert L.dppr_group_patch(e._h, gid, 0.0, 0.0, 0, 0, H, KEEP, None) == -1 and untouched()
    e.unmark(slot)
    out = eng.PatchOut(UO, I, P, DO, D, 55)
    for a in [(slot, 0.0, 0.0, cap, cap, H, EMITTED), (3, 0.0, 0.0, cap, cap, H, EMITTED), (-1, 0.0, 0.0, cap, cap, H, EMITTED)]:
        assert L.dppr_patch(e._h, *a, C.byref(out)) == -1 and out.written == 55 and untouched(), a
    assert_mark_is(e, h, 2, nows, s.marks[h], "rejected calls")  # the rejected calls left the group's mark alone
    # a valid call with caps above the totals writes exactly the totals
    assert L.dppr_group_patch(e._h, gid, 0.0, 0.0, cap, cap, H, KEEP, C.byref(out)) == 0 and out.written == 1
    want = ref.patch(nows, s.marks[h], 0.0, 0.0)
    ups, dels = int(want["up_offsets"][-1]), int(want["del_offsets"][-1])
    got = {"up_offsets": uo, "up_ids": ids[:ups], "up_p": p[:ups], "del_offsets": do, "del_ids": dl[:dels]}
    assert ups > 0 and ref.same_patch(got, want)
    assert np.all(ids[ups:] == -77) and np.all(p[ups:] == 3.25) and np.all(dl[dels:] == -78)
    e.close()


def test_existing_queries_are_untouched():
    s = Marked(1, widths=(3, 10))
    s.update(1)

    def snapshot():
        out = [s.e.export_sparse(s.slot, 1e-6, with_r=True), s.e.changes(s.slot, 8192, 0.0)[:3], s.e.topk(s.slot, 100, 0.0)]
        for gid in s.groups.values():
            out.append(s.e.group_export_sparse(gid, 1e-6, with_r=True))
            out += [x[:3] for x in s.e.group_changes(gid, 8192, 0.0)]
            out += s.e.group_topk(gid, 100)
        return out

    before = snapshot()
    for h, n in s.handles():
        for tau in thresholds(s.marks[h]):
            assert host_patch(s.e, h, tau, 1e-9, KEEP)["up_offsets"][-1] >= 0
    after = snapshot()
    assert len(after) == len(before)
    for a, b in zip(after, before):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    s.e.close()
