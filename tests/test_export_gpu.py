"""The exports (dppr_support / dppr_export_sparse / dppr_export_dense_dev and their group forms) against numpy over the dense
reads: for source i the entries are np.nonzero(p_i > min_p)[0] in that order, p and r at those ids compared by bit pattern;
a dense copy is the stack of the dense reads (astype(float32) for DPPR_F32), compared by bit pattern. Device memory comes from
the HIP runtime the library is already linked to (ctypes on the libamdhip64 of /proc/self/maps: no second runtime is loaded)."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests.test_changes_gpu import Marked, bits, star_slot
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

EPS = 1e-9
MIN_PS = (0.0, 1e-9, 1e-4, 1.0)
EX_TILE = 256
I64P = C.POINTER(C.c_int64)


class Hip:
    """alloc / free / fill / copy-back through the runtime that libdppr_hip.so brought in."""

    def __init__(self):
        eng.lib()
        paths = {l.rsplit(" ", 1)[-1].strip() for l in open("/proc/self/maps") if "libamdhip64" in l}
        assert len(paths) == 1, paths
        self.L = C.CDLL(paths.pop())
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipFree.argtypes = [C.c_void_p]
        self.L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.live = []

    def alloc(self, nbytes, fill=0xAB):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), max(int(nbytes), 8)) == 0
        assert self.L.hipMemset(p, fill, max(int(nbytes), 8)) == 0
        assert self.L.hipDeviceSynchronize() == 0  # (the fill is on the null stream and the engine's stream does not wait for that one)
        self.live.append(p.value)
        return p.value

    def read(self, ptr, nbytes, dtype=np.uint8):
        out = np.empty(int(nbytes), dtype=np.uint8)
        if nbytes:
            assert self.L.hipMemcpy(out.ctypes.data, ptr, int(nbytes), 2) == 0  # hipMemcpyDeviceToHost
        return out.view(dtype)

    def free_all(self):
        for p in self.live:
            assert self.L.hipFree(p) == 0
        self.live = []


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def cols_of(e, handle, n):
    """The dense reads: ([p_i], [r_i])."""
    if handle[0] == "slot":
        p, r = e.read(handle[1])
        return [p], [r]
    pr = [e.group_read(handle[1], i) for i in range(n)]
    return [x[0] for x in pr], [x[1] for x in pr]


def want_sparse(ps, rs, min_p):
    with np.errstate(invalid="ignore"):
        ids = [np.nonzero(p > min_p)[0] for p in ps]
    off = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int64)
    return (off, np.concatenate(ids).astype(np.int32), np.concatenate([p[i] for p, i in zip(ps, ids)]),
            np.concatenate([r[i] for r, i in zip(rs, ids)]))


def same_sparse(got, want, with_r, what):
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(bits(got[2]), bits(want[2])), what
    if with_r:
        assert np.array_equal(bits(got[3]), bits(want[3])), what


def export_dev(e, hip, handle, min_p, cap, with_r):
    """A device-destination export into fresh buffers of exactly cap entries: (offsets, ids, p, r or None) copied back."""
    d_ids, d_p = hip.alloc(4 * cap), hip.alloc(8 * cap)
    d_r = hip.alloc(8 * cap) if with_r else None
    fn = e.export_sparse_dev if handle[0] == "slot" else e.group_export_sparse_dev
    off = fn(handle[1], min_p, cap, d_ids, d_p, d_r)
    return off, hip.read(d_ids, 4 * cap, np.int32), hip.read(d_p, 8 * cap, np.float64), hip.read(d_r, 8 * cap, np.float64) if with_r else None


def check_sparse(e, hip, handle, n, ps, rs, min_ps=MIN_PS, what=""):
    totals = []
    for min_p in min_ps:
        want = want_sparse(ps, rs, min_p)
        total = int(want[0][n])
        totals.append(total)
        tag = (what, handle, n, min_p)
        sup = np.array([e.support(handle[1], min_p)]) if handle[0] == "slot" else e.group_support(handle[1], min_p)
        assert np.array_equal(sup, np.diff(want[0])), tag
        for with_r in (False, True):
            got = e.export_sparse(handle[1], min_p, with_r) if handle[0] == "slot" else e.group_export_sparse(handle[1], min_p, with_r)
            assert len(got) == (4 if with_r else 3)
            same_sparse(got, want, with_r, tag + ("host",))
            got = export_dev(e, hip, handle, min_p, total, with_r)
            same_sparse(got, want, with_r, tag + ("device",))
        hip.free_all()
    return totals


@pytest.mark.parametrize("directed", [1, 0])
def test_every_row_width(hip, directed):
    s = Marked(directed)
    for batches in (0, 3):  # after init_solve, and after 3 batches
        s.update(batches)
        for h, n in s.handles():
            ps, rs = cols_of(s.e, h, n)
            totals = check_sparse(s.e, hip, h, n, ps, rs, what=f"after {batches}")
            # 0.0: every positive entry; a larger min_p never admits more; 1.0: empty (p <= 1). Whether 1e-9 or 1e-4 cut anything
            # depends on the graph: that a threshold separates neighbouring doubles is test_tile_and_wave_edges_of_a_crafted_slot's
            assert totals[0] == sum(int(np.count_nonzero(p > 0)) for p in ps) and totals[0] >= totals[1] >= totals[2] > 0 and totals[3] == 0, (h, totals)
            off = (s.e.export_sparse(h[1], 1.0) if h[0] == "slot" else s.e.group_export_sparse(h[1], 1.0))[0]
            assert np.all(off == 0) and len(off) == n + 1
    s.e.close()


def test_capacity(hip):
    s = Marked(1, widths=(10,))
    s.update(1)
    e, gid, n = s.e, s.groups[10], 10
    L, hd = eng.lib(), e._h
    ps, rs = cols_of(e, ("group", gid), n)
    want = want_sparse(ps, rs, 1e-6)
    total = int(want[0][n])
    assert total > n
    # the size query: cap = 0, NULL arrays
    off = np.full(n + 1, -5, dtype=np.int64)
    for dest in (eng.DEST_HOST, eng.DEST_DEVICE):
        assert L.dppr_group_export_sparse(hd, gid, 1e-6, 0, dest, off.ctypes.data_as(I64P), None, None, None) == 0
        assert np.array_equal(off, want[0])
        off[:] = -5
    # host: cap = total fills, cap = total - 1 writes the offsets alone; a cap above n * V is as good as n * V
    for cap, fills in ((total, True), (total - 1, False), (total + 7, True), (1 << 40, True)):
        room = min(cap, total + 7)
        ids, p, r = np.full(room, -77, dtype=np.int32), np.full(room, 3.25), np.full(room, 4.5)
        off[:] = -5
        assert L.dppr_group_export_sparse(hd, gid, 1e-6, cap, eng.DEST_HOST, off.ctypes.data_as(I64P), ids.ctypes.data, p.ctypes.data, r.ctypes.data) == 0
        assert np.array_equal(off, want[0]), cap
        if fills:
            same_sparse((off, ids[:total], p[:total], r[:total]), want, True, ("host", cap))
            assert np.all(ids[total:] == -77) and np.all(p[total:] == 3.25) and np.all(r[total:] == 4.5)
        else:
            assert np.all(ids == -77) and np.all(p == 3.25) and np.all(r == 4.5)
    # device: the same, the sentinel is the 0xAB fill
    got = export_dev(e, hip, ("group", gid), 1e-6, total, True)
    same_sparse(got, want, True, "device, cap = total")
    got = export_dev(e, hip, ("group", gid), 1e-6, total - 1, True)
    assert np.array_equal(got[0], want[0])
    assert all(np.all(x.view(np.uint8) == 0xAB) for x in got[1:])
    e.close()


def test_tile_and_wave_edges_of_a_crafted_slot(hip):
    """States set by dppr_write: qualifying ids at the edges of the 256-id tiles and of the 64-lane waves and at V - 1, a tile that
    qualifies whole, an empty tile between two full ones; min_p itself, the next double above it, -0.0, a negative value and NaN
    around them: only the second qualifies."""
    V = 5 * EX_TILE
    e, slot, _ = star_slot(10, V)
    min_p = 0.25
    above = np.nextafter(min_p, np.inf)
    edges = [63, 64, 65, V - 1] + [t * EX_TILE - 1 for t in range(1, 5)] + [t * EX_TILE for t in range(1, 5)]
    full = list(range(EX_TILE, 2 * EX_TILE)) + list(range(3 * EX_TILE, 4 * EX_TILE)) + [5, 70, 4 * EX_TILE + 9, V - 1]  # tile 2 stays empty
    others = [min_p, -0.0, -1.5, float("nan"), 0.0]
    rng = np.random.default_rng(7)
    for name, qual in (("edges", edges), ("full and empty tiles", full)):
        p = np.array([others[v % len(others)] for v in range(V)])
        p[qual] = above
        r = np.where(p != 0.0, rng.standard_normal(V), 0.0)  # (a vertex whose p and r are zero gets no id)
        e.write(slot, p, r)
        ps, rs = cols_of(e, ("slot", slot), 1)
        assert np.array_equal(np.isnan(ps[0]), np.isnan(p)) and np.count_nonzero(ps[0] < 0) == np.count_nonzero(p < 0)
        got = e.export_sparse(slot, min_p, with_r=True)
        assert np.array_equal(got[1], np.sort(np.unique(qual))), name  # only `above` qualifies
        assert np.all(got[2] == above)
        sp = e.id_space()
        assert sp["ids"] + sp["parked"] < V  # (the -0.0 and 0.0 vertices never got an id)
        totals = check_sparse(e, hip, ("slot", slot), 1, ps, rs, min_ps=(min_p, 0.0, above), what=name)
        assert totals[0] == len(set(qual)) and totals[1] == totals[0] + np.count_nonzero(p == min_p) and totals[2] == 0
    e.close()


def test_parked_zone_and_renumbering(hip):
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
    before = e.id_space()
    handles = ((("slot", slot), 1), (("group", gid), 10))
    first = {}
    for h, n in handles:
        ps, rs = cols_of(e, h, n)
        check_sparse(e, hip, h, n, ps, rs, min_ps=(0.0, 1e-6), what="before")
        first[h] = ps
    for _ in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.update(slot, EPS)
        e.group_update(gid, EPS)
    sp = e.id_space()
    assert sp["renumberings"] > before["renumberings"] and sp["parked"] > 0 and sp["revivals"] > 0, (before, sp)
    for h, n in handles:
        ps, rs = cols_of(e, h, n)
        check_sparse(e, hip, h, n, ps, rs, min_ps=(0.0, 1e-6), what="after")
        ids = e.export_sparse(slot, 0.0)[1] if h[0] == "slot" else e.group_export_sparse(gid, 0.0)[1]
        in_window = np.zeros(V, dtype=bool)
        w1, w2 = g.window_edges()
        in_window[w1] = in_window[w2] = True
        gone = np.unique(ids[~in_window[ids]])
        assert len(np.setdiff1d(gone, np.arange(10))) > 0  # entries of vertices that have left the window: rows outside the live graph
        was = np.zeros(V, dtype=bool)
        for col in first[h]:
            was |= col > 0
        assert np.any(was[ids]) and np.any(~was[ids])  # vertices that were there before the renumbering, and new ones
    e.close()


def test_churn_of_the_sources_changes_the_lane_order(hip):
    s = Marked(1, widths=(8,))
    e, gid = s.e, s.groups[8]
    idx, _ = e.group_add_source(gid, s.srcs[8])  # 8 -> 9: the row width switches
    assert idx == 8 and e.group_sources(gid) == s.srcs[:9]
    ps, rs = cols_of(e, ("group", gid), 9)
    assert ps[8][s.srcs[8]] > 0
    check_sparse(e, hip, ("group", gid), 9, ps, rs, min_ps=(0.0, 1e-4), what="after add")
    e.group_remove_source(gid, 0)
    assert e.group_sources(gid) == s.srcs[1:9]
    ps, rs = cols_of(e, ("group", gid), 8)
    check_sparse(e, hip, ("group", gid), 8, ps, rs, min_ps=(0.0, 1e-4), what="after remove")
    e.close()


def test_dense(hip):
    s = Marked(0, widths=(1, 3, 10, 16))
    s.update(1)
    e, V = s.e, s.V
    sp = e.id_space()
    assert sp["ids"] + sp["parked"] < V  # some vertex has no id: its entries are 0.0
    for h, n in s.handles():
        ps, rs = cols_of(e, h, n)
        assert any(np.all(col == 0.0) for col in np.stack(ps, axis=1))
        for which, cols in ((eng.DENSE_P, ps), (eng.DENSE_R, rs)):
            for dtype, np_t, np_u in ((eng.F64, np.float64, np.uint64), (eng.F32, np.float32, np.uint32)):
                for layout in ((eng.VERTEX_MAJOR,) if h[0] == "slot" else (eng.VERTEX_MAJOR, eng.SOURCE_MAJOR)):
                    want = np.ascontiguousarray(np.stack(cols, axis=0 if layout == eng.SOURCE_MAJOR else 1).astype(np_t))
                    nbytes = want.nbytes
                    dst = hip.alloc(nbytes + 16)
                    if h[0] == "slot":
                        e.export_dense_dev(h[1], dst, which, dtype)
                    else:
                        e.group_export_dense_dev(h[1], dst, which, dtype, layout)
                    raw = hip.read(dst, nbytes + 16)
                    assert np.array_equal(raw[:nbytes].view(np_u), want.reshape(-1).view(np_u)), (h, n, which, dtype, layout)
                    assert np.all(raw[nbytes:] == 0xAB), (h, n, which, dtype, layout)
        hip.free_all()
    e.close()


def test_rejections_write_nothing(hip):
    s = Marked(1, widths=(3,))
    e, gid, slot, n, V = s.e, s.groups[3], s.slot, 3, s.V
    L, hd = eng.lib(), e._h
    total = int(e.group_support(gid, 0.0).sum())
    off = np.full(n + 1, -5, dtype=np.int64)
    O = off.ctypes.data_as(I64P)
    ids, p, r = np.full(total, -77, dtype=np.int32), np.full(total, 3.25), np.full(total, 4.5)
    d_ids, d_p, d_r = hip.alloc(4 * total), hip.alloc(8 * total), hip.alloc(8 * total)
    short_p, short_ids = hip.alloc(8 * total - 8), hip.alloc(4 * total - 4)

    def untouched():
        dev = [hip.read(x, nb) for x, nb in ((d_ids, 4 * total), (d_p, 8 * total), (d_r, 8 * total), (short_p, 8 * total - 8), (short_ids, 4 * total - 4))]
        return np.all(off == -5) and np.all(ids == -77) and np.all(p == 3.25) and np.all(r == 4.5) and all(np.all(x == 0xAB) for x in dev)

    H, D = eng.DEST_HOST, eng.DEST_DEVICE
    I, P, R = ids.ctypes.data, p.ctypes.data, r.ctypes.data
    nan = float("nan")
    bad = [(gid, -1.0, total, H, O, I, P, R), (gid, -1e-300, total, H, O, I, P, R), (gid, nan, total, H, O, I, P, R), (gid, nan, 0, H, O, None, None, None),
           (gid, 0.0, -1, H, O, I, P, R), (gid, 0.0, total, H, None, I, P, R), (gid, 0.0, 0, H, None, None, None, None),
           (gid, 0.0, total, H, O, None, P, R), (gid, 0.0, total, H, O, I, None, R), (gid, 0.0, total, 2, O, I, P, R), (gid, 0.0, total, -1, O, I, P, R),
           (7, 0.0, total, H, O, I, P, R), (-1, 0.0, total, H, O, I, P, R),
           # a device destination: a host pointer, NULL, one element too short, misaligned
           (gid, 0.0, total, D, O, I, d_p, d_r), (gid, 0.0, total, D, O, d_ids, P, d_r), (gid, 0.0, total, D, O, d_ids, d_p, R),
           (gid, 0.0, total, D, O, None, d_p, d_r), (gid, 0.0, total, D, O, d_ids, None, d_r),
           (gid, 0.0, total, D, O, d_ids, short_p, d_r), (gid, 0.0, total, D, O, short_ids, d_p, d_r), (gid, 0.0, total, D, O, d_ids, d_p, short_p),
           (gid, 0.0, total - 1, D, O, d_ids + 2, d_p, d_r), (gid, 0.0, total - 1, D, O, d_ids, d_p + 4, d_r), (gid, 0.0, total - 1, D, O, d_ids, d_p, d_r + 4),
           (gid, 0.0, total - 1, D, O, d_ids + 4, d_p, d_r + 8 * total)]  # (the last: r begins where its allocation ends)
    for a in bad:
        assert L.dppr_group_export_sparse(hd, *a) == -1, a
        assert untouched(), a
    for a in [(3, 0.0, total, H, O, I, P, R), (-1, 0.0, 0, H, O, None, None, None), (slot, -1.0, 0, H, O, None, None, None),
              (slot, 0.0, V, D, O, I, d_p, None), (slot, 0.0, V, 5, O, I, P, None)]:
        assert L.dppr_export_sparse(hd, *a) == -1, a
        assert untouched(), a
    for a in [(gid, -1.0, O), (gid, nan, O), (gid, 0.0, None), (7, 0.0, O), (-1, 0.0, O)]:
        assert L.dppr_group_support(hd, *a) == -1, a
    for a in [(slot, -1.0, O), (slot, nan, O), (slot, 0.0, None), (3, 0.0, O)]:
        assert L.dppr_support(hd, *a) == -1, a
    assert untouched()
    # dense
    nb = 8 * n * V
    dst, short = hip.alloc(nb + 16), hip.alloc(nb - 8)
    host = np.full(n * V, 3.25)
    P0, F64, F32, VM, SM = eng.DENSE_P, eng.F64, eng.F32, eng.VERTEX_MAJOR, eng.SOURCE_MAJOR
    for a in [(gid, 2, F64, VM, dst), (gid, -1, F64, VM, dst), (gid, P0, 2, VM, dst), (gid, P0, -1, SM, dst), (gid, P0, F64, 2, dst), (gid, P0, F64, -1, dst),
              (7, P0, F64, VM, dst), (-1, P0, F64, VM, dst), (gid, P0, F64, VM, None), (gid, P0, F64, SM, host.ctypes.data),
              (gid, P0, F64, VM, short), (gid, P0, F64, SM, short), (gid, P0, F64, VM, dst + 4), (gid, P0, F32, SM, dst + 2),
              (gid, P0, F64, VM, dst + 24), (gid, P0, F32, VM, dst + nb // 2 + 20)]:
        assert L.dppr_group_export_dense_dev(hd, *a) == -1, a
    for a in [(3, P0, F64, dst), (slot, 2, F64, dst), (slot, P0, 2, dst), (slot, P0, F64, None), (slot, P0, F64, host.ctypes.data), (slot, P0, F64, dst + nb + 16 - 8 * V + 8)]:
        assert L.dppr_export_dense_dev(hd, *a) == -1, a
    assert np.all(hip.read(dst, nb + 16) == 0xAB) and np.all(hip.read(short, nb - 8) == 0xAB) and np.all(host == 3.25)
    # the same buffers are good for the calls that fit them
    assert L.dppr_group_export_dense_dev(hd, gid, P0, F32, SM, short) == 0
    assert L.dppr_group_export_sparse(hd, gid, 0.0, total, D, O, d_ids, d_p, d_r) == 0 and off[n] == total
    e.close()


def test_bystanders_are_untouched(hip):
    s = Marked(1, widths=(10,))
    s.update(1)
    e, gid = s.e, s.groups[10]

    def snapshot():
        out = [x for k in (10, 8192) for t in e.group_topk(gid, k) for x in t]
        out += [np.asarray(x) for t in e.group_changes(gid, 100) for x in t]
        out += [x for i in range(10) for x in e.group_read(gid, i)]
        return out

    before = snapshot()
    ps, rs = cols_of(e, ("group", gid), 10)
    check_sparse(e, hip, ("group", gid), 10, ps, rs, min_ps=(0.0, 1e-6))
    dst = hip.alloc(8 * 10 * s.V)
    e.group_export_dense_dev(gid, dst, eng.DENSE_R, eng.F64, eng.SOURCE_MAJOR)
    e.group_export_dense_dev(gid, dst, eng.DENSE_P, eng.F32, eng.VERTEX_MAJOR)
    after = snapshot()
    assert len(after) == len(before)
    for a, b in zip(after, before):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8) if a.ndim else a, b.view(np.uint8) if b.ndim else b)
    e.close()


def test_buffers_go_with_the_engine(hip):
    gc.collect()
    before = eng.live_bytes()
    s = Marked(1, widths=(10,))
    gid = s.groups[10]
    held = eng.live_bytes()
    assert s.e.group_support(gid, 0.0).sum() > 0
    with_ws = eng.live_bytes()
    assert with_ws[0] > held[0] and with_ws[1] > held[1]  # the work space and the head of the block, device and pinned
    s.e.group_export_sparse(gid, 0.0, with_r=True)
    grown = eng.live_bytes()
    assert grown[0] > with_ws[0] and grown[1] > with_ws[1]  # the block of a host destination grew with cap
    s.e.group_export_sparse(gid, 1e-4, with_r=True)
    s.e.export_sparse(s.slot, 0.0)
    assert eng.live_bytes() == grown  # a smaller export takes nothing new
    dst = hip.alloc(8 * 10 * s.V)
    s.e.group_export_dense_dev(gid, dst)
    assert eng.live_bytes() == grown  # the dense export needs no buffer of the engine's
    s.e.close()
    gc.collect()
    assert eng.live_bytes() == before
