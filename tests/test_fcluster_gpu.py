"""The full-length conductance sweep of a forward track (dppr_ftrack_cluster) on the device against the numpy definition of
tests/fcluster_ref.py: the track's p from tests/ftrack_ref.py, the epoch's out-rows from dppr_read_out_graph. Ids, prefix arrays and
the records are compared as integers, scores and phi by bit pattern. The fixtures are those of tests/test_ftrack_gpu.py: the R-MAT
scale-10 stream, V = 1024, 4000 window edges."""
import ctypes as C

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from tests import fcluster_ref as fcr
from tests.test_export_gpu import Hip
from tests.test_forward_gpu import bits, star
from tests.test_fpush_gpu import WIDTHS
from tests.test_ftrack_gpu import RefTrack, Window, standard_sets

pytestmark = pytest.mark.gpu

ORDERS = ("deg", "p")
NAMES = ("ids", "score", "cut_out", "cut_in", "vol")
DTYPES = (np.int32, np.float64, np.int64, np.int64, np.int64)


def out_graph(e, epoch=-1):
    row, col = e.read_out_graph(epoch)
    return row.astype(np.int64), col.astype(np.int64)[:int(row[-1])]


def columns_of(got):
    """The (best, ids, score, cut_out, cut_in, vol) of every column of a ForwardTrack.cluster(profile=True) result."""
    best, off = got[0], got[1]
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and all(len(a) == off[-1] for a in got[2:])
    return [(best[c], *[a[off[c]:off[c + 1]] for a in got[2:]]) for c in range(len(best))]


class Want:
    """The reference results of one epoch, computed once per (column state, arguments)."""

    def __init__(self, e):
        self.row, self.col = out_graph(e)
        self.memo = {}

    def __call__(self, column, order, min_score=0.0, max_len=0, min_size=1):
        key = (id(column), column.p.tobytes(), order, min_score, max_len, min_size)
        if key not in self.memo:
            self.memo[key] = fcr.cluster(column.p, self.row, self.col, order, min_score, max_len, min_size)
        return self.memo[key]


def check(what, t, cols, want, order, **kw):
    got = columns_of(t.cluster(order, profile=True, **kw))
    assert len(got) == len(cols)
    for i, (g, c) in enumerate(zip(got, cols)):
        fcr.same(g, want(c, order, **kw), (what, order, i))
    return got


def blob(got):
    return b"".join([b"".join(repr(sorted(b.items())).encode() + np.float64(b["best_phi"]).tobytes() for b in got[0])] +
                    [np.ascontiguousarray(a).tobytes() for a in got[1:]])


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_both_orders_after_the_create_and_after_every_batch(directed):
    w = Window(directed)
    e = w.e
    sets, who = standard_sets(w)
    tracks = []
    for eps, cap in ((1e-6, 64), (1e-8, 5)):   # (five rounds leave the second unconverged)
        ref = RefTrack(w.rows, sets, eps, cap)
        tracks.append((ref, {m: e.ftrack(sets[:m], eps, cap) for m in WIDTHS}))
    want = Want(e)
    for ref, by_m in tracks:
        for m, t in by_m.items():
            for order in ORDERS:
                got = check((directed, "create", m), t, ref.cols[:m], want, order)
                if m == 16:   # the rowless rule: the never-named vertex holds p = 0.15 w and is in no order; its own column is empty
                    assert ref.cols[2].p[who["unnamed"]] == 0.15 and got[2][0]["count"] == 0 and got[2][0]["best_phi"] == float("inf")
                    assert all(who["unnamed"] not in g[1] for g in got) and ref.cols[4].p[who["unnamed"]] > 0
                    assert max(g[0]["count"] for g in got) > 256
    signed = 0
    for b in range(6):
        rec, rows = w.slide()
        want = Want(e)
        for ref, by_m in tracks:
            ref.update(rows, rec, 64)
            signed += int(any(np.any(c.p < 0) for c in ref.cols))
            for m, t in by_m.items():
                t.update(w.epoch, 64)
                if m in (16, 5) or b == 5:
                    for order in ORDERS:
                        got = check((directed, b, m), t, ref.cols[:m], want, order)
                        if not directed:
                            assert all(np.array_equal(g[3], g[4]) for g in got), "both directions stored: cut_in == cut_out"
    assert signed > 0   # an update makes p signed: negative scores never qualify
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_hook_changes_no_bit():
    w = Window(0)
    e = w.e
    sets, who = standard_sets(w)
    t = e.ftrack(sets, 1e-6, 64)
    for _ in range(2):
        w.slide()
        t.update(w.epoch, 64)
    assert w.rows.d.max() > 64   # piece_edges = 64 cuts the hub's rows into pieces
    first = {}
    for tile, piece in ((0, 0), (64, 64), (64, 0), (0, 64), (4096, 4096), (128, 256), (0, 0)):
        e.debug_ftrack_cluster(tile, piece)
        for order in ORDERS:
            a = t.cluster(order, profile=True)
            assert max(b["count"] for b in a[0]) > 3 * 64   # scan_tile = 64: several tiles and a carry
            z = t.cluster(order, profile=True)
            assert blob(a) == blob(z), "two calls in a row"
            assert blob(a) == first.setdefault(order, blob(a)), (tile, piece, order)
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_ties_in_id_order_and_a_row_longer_than_every_piece():
    D = 4200   # the in-row of vertex 0 and the out-row of S: longer than the largest piece (4096)
    V, tails, heads, S = star(D)
    tails, heads = tails[::-1].copy(), heads[::-1].copy()   # the leaves enter the stream in DESCENDING id
    e = eng.Engine(V, len(tails), 1, 1)
    e.load_window(tails, heads)
    x2i = e.id_map()
    assert np.all(x2i[1:D + 1] >= 0) and not np.all(np.diff(x2i[1:D + 1]) > 0)   # internal and external order differ
    row, col = out_graph(e)
    assert row[S + 1] - row[S] == D and np.sum(col == 0) == D
    from tests import forward_ref as fr
    from tests import ftrack_ref as tr
    rows = fr.Rows(V, *e.read_graph()[:2], x2i)
    column = tr.Column(rows, [S], [1.0], 1e-7, 6)
    leaves = column.p[1:D + 1]
    assert leaves[0] > 0 and np.all(bits(leaves) == bits(leaves[:1]))   # every leaf ties under BY_P
    t = e.ftrack([S], 1e-7, 6)
    first = None
    for tile, piece in ((0, 0), (64, 64), (4096, 4096)):
        e.debug_ftrack_cluster(tile, piece)
        for order in ORDERS:
            want = fcr.cluster(column.p, row, col, order)
            got = columns_of(t.cluster(order, profile=True))[0]
            fcr.same(got, want, (tile, piece, order))
            if order == "p":
                where = np.nonzero(got[1] == 1)[0][0]
                assert np.array_equal(got[1][where:where + D], np.arange(1, D + 1)), "the ties stand in external id order"
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def two_cliques(n=40):
    a = [(i, j) for i in range(n) for j in range(i + 1, n)]
    edges = a + [(i + n, j + n) for i, j in a] + [(n - 1, n)]
    return 2 * n, np.array([x for x, _ in edges], dtype=np.int32), np.array([y for _, y in edges], dtype=np.int32)


PLANTED_EPS = 1e-6


def test_a_planted_cut_is_found():
    V, t1, t2 = two_cliques()
    e = eng.Engine(V, len(t1), 0, 1)
    e.load_window(t1, t2)
    row, col = out_graph(e)
    assert row[-1] == 2 * len(t1)
    from tests import forward_ref as fr
    from tests import ftrack_ref as tr
    column = tr.Column(fr.Rows(V, *e.read_graph()[:2], e.id_map()), [0], [1.0], PLANTED_EPS, 64)
    want = fcr.cluster(column.p, row, col, "deg")
    # on the REFERENCE alone: the best prefix is exactly the start's clique, cut by the one bridge
    assert want[0]["best_size"] == 40 and sorted(want[1][:40].tolist()) == list(range(40))
    assert want[0]["best_cut"] == 1 and want[0]["best_vol"] == 40 * 39 + 1 and want[0]["best_phi"] == 1.0 / 1561.0
    t = e.ftrack([0], PLANTED_EPS, 64)
    got = columns_of(t.cluster("deg", profile=True))[0]
    fcr.same(got, want, "planted")
    assert t.cluster("deg")[0] == got[0]
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_prefix_property_top_k_agreement_and_arguments():
    w = Window(1)
    e = w.e
    sets, who = standard_sets(w)
    t, ref = e.ftrack(sets[:6], 1e-6, 64), RefTrack(w.rows, sets[:6], 1e-6, 64)
    rec, rows = w.slide()
    ref.update(rows, rec, 64)
    t.update(w.epoch, 64)
    want = Want(e)
    named = (np.diff(want.row) > 0) | (np.bincount(want.col, minlength=w.V) > 0)
    for order in ORDERS:
        full = check("full", t, ref.cols, want, order)
        head = check("max_len 37", t, ref.cols, want, order, max_len=37)
        for f, h in zip(full, head):
            L = min(37, len(f[1]))
            assert h[0]["count"] == L and all(np.array_equal(np.asarray(a[:L]).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(f[1:], h[1:]))
        check("min_score", t, ref.cols, want, order, min_score=1e-5, min_size=4)
        check("max_len V", t, ref.cols, want, order, max_len=w.V, min_size=500)
    # BY_P: the order opens with the top k of the read, once the seeds that no edge names are removed
    top = t.read(k=60)["topk"]
    got = columns_of(t.cluster("p", profile=True))
    for i, ((ids, p), g) in enumerate(zip(top, got)):
        keep = named[ids]
        assert np.array_equal(ids[keep], g[1][:keep.sum()]) and np.array_equal(bits(p[keep]), bits(g[2][:keep.sum()])), i
    assert not named[who["unnamed"]] and who["unnamed"] in top[2][0] and who["unnamed"] in top[4][0]
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_capacity_and_device_destinations():
    w = Window(0)
    e = w.e
    hip = Hip()
    sets, _ = standard_sets(w)
    t = e.ftrack(sets[:5], 1e-6, 64)
    host = t.cluster("deg", profile=True)
    total = int(host[1][-1])
    assert total > 1000
    sizes = [np.dtype(d).itemsize for d in DTYPES]
    for cap in (total - 1, total, total + 7, 0):
        ptrs = {n: hip.alloc(s * max(cap, 1) + 16) for n, s in zip(NAMES, sizes)}
        best, off = t.cluster("deg", device_ptrs=ptrs, cap=cap)
        assert best == host[0] and np.array_equal(off, host[1]), cap   # always written, with the TRUE counts
        for n, s, d, a in zip(NAMES, sizes, DTYPES, host[2:]):
            raw = hip.read(ptrs[n], s * max(cap, 1) + 16)
            if cap < total:
                assert np.all(raw == 0xAB), (cap, n, "nothing is written when the entries do not fit")
            else:
                assert np.array_equal(raw[:s * total], np.ascontiguousarray(a).view(np.uint8)), (cap, n)
                assert np.all(raw[s * total:] == 0xAB), (cap, n, "past the entries")
        hip.free_all()
    # some arrays only
    ptrs = {"ids": hip.alloc(4 * total), "vol": hip.alloc(8 * total)}
    best, off = t.cluster("deg", device_ptrs=ptrs, cap=total)
    assert best == host[0] and np.array_equal(hip.read(ptrs["ids"], 4 * total, np.int32), host[2]) and np.array_equal(hip.read(ptrs["vol"], 8 * total, np.int64), host[6])
    # the size-and-best query
    assert t.cluster("deg") == host[0]
    hip.free_all()
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_track_and_the_outputs_untouched():
    w = Window(1, n_epochs=2)
    e, V = w.e, w.V
    hip = Hip()
    L, h = e._L, e._h
    sets, _ = standard_sets(w)
    t = e.ftrack(sets[:2], 1e-6, 8)
    at = np.arange(V, dtype=np.int32)
    state = t.read(at=at)
    cap = 2 * V
    best, off = np.full(5 * 16, 77, dtype=np.int64), np.full(17, 77, dtype=np.int64)
    host = {n: np.full(cap, 77, dtype=d) for n, d in zip(NAMES, DTYPES)}
    dev = {n: hip.alloc(np.dtype(d).itemsize * cap) for n, d in zip(NAMES, DTYPES)}
    small = hip.alloc(64)

    def clean():
        return bool(np.all(best == 77) and np.all(off == 77) and all(np.all(a == 77) for a in host.values()) and
                    all(np.all(hip.read(p, 4 * cap) == 0xAB) for p in dev.values()) and t.info()["epoch"] == 0 and
                    all(np.asarray(now).tobytes() == np.asarray(state[k]).tobytes() for k, now in t.read(at=at).items()))

    def refused(track=None, order=1, min_score=0.0, max_len=0, min_size=1, cap=cap, dest=eng.DEST_HOST, b=best.ctypes.data, o=off.ctypes.data, arrays="host"):
        if arrays == "host":
            arrays = [host[n].ctypes.data for n in NAMES]
        elif arrays == "dev":
            arrays = [dev[n] for n in NAMES]
        rc = L.dppr_ftrack_cluster(h, t.handle if track is None else track, order, min_score, max_len, min_size, cap, dest, b, o, *arrays)
        return rc == -1 and clean()

    for kw in (dict(track=-1), dict(track=16), dict(track=t.handle + 1), dict(order=2), dict(order=-1), dict(min_score=-1e-300),
               dict(min_score=float("nan")), dict(max_len=-1), dict(max_len=V + 1), dict(min_size=0), dict(min_size=-3), dict(cap=-1),
               dict(arrays=[None] * 5), dict(dest=2), dict(dest=-1), dict(b=None), dict(o=None),
               dict(dest=eng.DEST_DEVICE, arrays="host"),                                  # host memory as a device destination
               dict(dest=eng.DEST_DEVICE, arrays=[dev["ids"] + 2, None, None, None, None]),  # misaligned
               dict(dest=eng.DEST_DEVICE, arrays=[None, None, dev["cut_out"] + 4, None, None]),
               dict(dest=eng.DEST_DEVICE, arrays=[None, small, None, None, None]),          # an allocation that cannot hold cap entries
               dict(dest=eng.DEST_DEVICE, arrays=[dev["ids"], dev["score"], dev["cut_out"], dev["cut_in"], dev["vol"] + 8])):
        assert refused(**kw), list(kw)
    # (the good calls are good: the same arguments without the fault are accepted)
    assert L.dppr_ftrack_cluster(h, t.handle, 1, 0.0, 0, 1, cap, eng.DEST_DEVICE, best.ctypes.data, off.ctypes.data, *[dev[n] for n in NAMES]) == 0
    assert L.dppr_ftrack_cluster(h, t.handle, 1, 0.0, 0, 1, 0, 0, best.ctypes.data, off.ctypes.data, None, None, None, None, None) == 0
    assert off[0] == 0 and 0 < off[2] <= cap and np.all(hip.read(dev["ids"], 4 * int(off[2]), np.int32) >= 0)
    best[:], off[:] = 77, 77
    for p, d in zip(dev.values(), DTYPES):
        hip.L.hipMemset(p, 0xAB, np.dtype(d).itemsize * cap)
    assert hip.L.hipDeviceSynchronize() == 0
    w.slide()
    w.slide()   # epochs 1 and 2 are resident (n_epochs = 2): the track's epoch 0 is not
    assert refused() and refused(dest=eng.DEST_DEVICE, arrays="dev"), "the track's epoch is no longer resident"
    hip.free_all()
    e.close()
