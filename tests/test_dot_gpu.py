"""The dot products over the vertex axis (dppr_dot_dense_dev / dppr_dot_sparse and their group forms) against the numpy fold of
tests/dot_ref.py over the dense reads, compared by bit pattern: there is no tolerance anywhere. Device memory comes from the HIP
runtime the library is already linked to (the Hip helper of tests/test_export_gpu.py)."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests import dot_ref
from tests.test_changes_gpu import WIDTHS, Marked, bits, star_slot
from tests.test_export_gpu import Hip, cols_of
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

EPS = 1e-9
I64P = C.POINTER(C.c_int64)
P, R = eng.DENSE_P, eng.DENSE_R
FM, VM = eng.H_FEATURE_MAJOR, eng.H_VERTEX_MAJOR
QUARTET = np.array([1e16, 1.0, -1e16, 1.0])


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def put(hip, a):
    """A host array in fresh device memory: the raw address."""
    a = np.ascontiguousarray(a)
    ptr = hip.alloc(a.nbytes)
    if a.nbytes:
        assert hip.L.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
    return ptr


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), (what, got.ravel()[:4], want.ravel()[:4])


def dense_call(e, hip, handle, n, h, which=P, dtype=eng.F64, layout=FM, dest="host"):
    """h: [F][V] float64 or float32, the logical features; uploaded in `layout`. The scores [F][n]."""
    F = h.shape[0]
    d_h = put(hip, h if layout == FM else h.T)
    fn = e.dot_dense_dev if handle[0] == "slot" else e.group_dot_dense_dev
    if dest == "host":
        out = fn(handle[1], d_h, F, which, dtype, layout)
    else:
        d_out = hip.alloc(8 * F * n + 16)
        assert fn(handle[1], d_h, F, which, dtype, layout, out_ptr=d_out) is None
        raw = hip.read(d_out, 8 * F * n + 16)
        assert np.all(raw[8 * F * n:] == 0xAB)
        out = raw[:8 * F * n].view(np.float64)
    return np.asarray(out).reshape(F, n)


def sparse_call(e, hip, handle, n, off, ids, w, which=P, src="host", dest="host"):
    F = len(off) - 1
    if src == "host":
        fn = e.dot_sparse if handle[0] == "slot" else e.group_dot_sparse
        a = (off, ids, w)
    else:
        fn = e.dot_sparse_dev if handle[0] == "slot" else e.group_dot_sparse_dev
        a = (off, put(hip, np.asarray(ids, dtype=np.int32)), put(hip, np.asarray(w, dtype=np.float64)))
    if dest == "host":
        out = fn(handle[1], *a, which)
    else:
        d_out = hip.alloc(8 * F * n + 16)
        assert fn(handle[1], *a, which, out_ptr=d_out) is None
        raw = hip.read(d_out, 8 * F * n + 16)
        assert np.all(raw[8 * F * n:] == 0xAB)
        out = raw[:8 * F * n].view(np.float64)
    return np.asarray(out).reshape(F, n)


def csr_of(h, thr):
    """The entries of every feature with |h| > thr, in id order."""
    ids = [np.nonzero(np.abs(row) > thr)[0] for row in h]
    off = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int64)
    return off, np.concatenate(ids).astype(np.int32), np.concatenate([row[i] for row, i in zip(h, ids)])


def star(V, L):
    """star_slot without its demand for a shuffled order (a star of one leaf has none)."""
    if L >= 2:
        return star_slot(L, V)
    e = eng.Engine(V, L, 0, 1, schedule=eng.SCHEDULE_SYNC)
    e.load_window(np.zeros(L, dtype=np.int32), np.arange(1, L + 1, dtype=np.int32))
    return e, e.add_source(0), np.arange(L + 1, dtype=np.int64)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_every_row_width(hip, directed):
    s = Marked(directed)
    V = s.V
    rng = np.random.default_rng(21)
    hs = {F: rng.standard_normal((F, V)) for F in (1, 16, 17)}
    assert all(np.any(h > 0) and np.any(h < 0) for h in hs.values())
    for batches in (0, 3):
        s.update(batches)
        for hd, n in s.handles():
            ps, rs = cols_of(s.e, hd, n)
            assert n in (1,) + WIDTHS
            for which, cols in ((P, ps), (R, rs)):
                for F, h in hs.items():
                    want = dot_ref.dense(h, cols)
                    for dest in ("host", "device"):
                        same(dense_call(s.e, hip, hd, n, h, which, dest=dest), want, (batches, hd, n, which, F, dest))
                    off, ids, w = csr_of(h, 0.8)
                    assert 0 < len(ids) < F * V
                    wsp = dot_ref.sparse(off, ids, w, cols)
                    same(sparse_call(s.e, hip, hd, n, off, ids, w, which, "host", "host"), wsp, (batches, hd, n, which, F, "sparse host"))
                    same(sparse_call(s.e, hip, hd, n, off, ids, w, which, "device", "device"), wsp, (batches, hd, n, which, F, "sparse dev"))
                hip.free_all()
    s.e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_layouts_and_dtypes(hip):
    s = Marked(1, widths=(10,))
    s.update(1)
    hd, n = ("group", s.groups[10]), 10
    ps, _ = cols_of(s.e, hd, n)
    rng = np.random.default_rng(22)
    for F in (1, 15, 16, 33):
        h = rng.standard_normal((F, s.V))
        for dtype, np_t in ((eng.F64, np.float64), (eng.F32, np.float32)):
            ht = h.astype(np_t)
            want = dot_ref.dense(ht.astype(np.float64), ps)
            for layout in (FM, VM):
                for dest in ("host", "device"):
                    same(dense_call(s.e, hip, hd, n, ht, P, dtype, layout, dest), want, (F, dtype, layout, dest))
        hip.free_all()
    s.e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_order_is_the_tree(hip):
    V = 65536 + 600
    e, slot, verts = star_slot(300, V)
    spots = (8, 255, 65535)  # four neighbouring ids: inside a subtile, across a 256-slot boundary, across a block boundary
    p = np.zeros(V)
    p[verts] = 1.0
    for at in spots:
        p[at:at + 4] = 1.0
    e.write(slot, p, np.zeros(V))
    ps, _ = cols_of(e, ("slot", slot), 1)
    assert np.array_equal(ps[0], p)
    for at in spots:
        h = np.zeros((1, V))
        h[0, at:at + 4] = QUARTET
        want = dot_ref.dense(h, ps)
        if at % 2 == 0:  # the quartet is two pairs of the tree: (1e16 + 1) + (-1e16 + 1) loses both ones
            assert want[0, 0] == 0.0 and dot_ref.running(h[0] * p) == 1.0 and float(np.dot(h[0], p)) == 2.0
        assert want[0, 0] != dot_ref.running(h[0] * p)
        same(dense_call(e, hip, ("slot", slot), 1, h), want, ("dense", at))
        off, ids, w = csr_of(h, 0.0)
        assert list(ids) == list(range(at, at + 4))
        # the slots of a sparse query are its entries: the same quartet at entries 0..3 is the aligned case wherever the ids lie
        got = sparse_call(e, hip, ("slot", slot), 1, off, ids, w)
        assert got[0, 0] == 0.0
        same(got, dot_ref.sparse(off, ids, w, ps), ("sparse", at))
        # ... and behind `at` entries of weight zero it sits at the slots the dense call has it at
        ids2 = np.concatenate([np.zeros(at, dtype=np.int32), ids]).astype(np.int32)
        w2 = np.concatenate([np.zeros(at), w])
        off2 = np.array([0, len(ids2)], dtype=np.int64)
        got = sparse_call(e, hip, ("slot", slot), 1, off2, ids2, w2, src="device")
        same(got, want, ("sparse at the same slots", at))
        hip.free_all()
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1 + 1, 255, 256, 257, 65536 + 257])
def test_tile_and_block_edges(hip, V):
    e, slot, verts = star(V, min(600, V - 1))
    rng = np.random.default_rng(V)
    p, r = np.zeros(V), np.zeros(V)
    p[verts], r[verts] = rng.standard_normal(len(verts)), rng.standard_normal(len(verts))
    e.write(slot, p, r)
    hd = ("slot", slot)
    ps, rs = cols_of(e, hd, 1)
    for F in (1, 3):
        h = rng.standard_normal((F, V)) * np.exp(3 * rng.standard_normal((F, V)))
        for which, cols in ((P, ps), (R, rs)):
            same(dense_call(e, hip, hd, 1, h, which), dot_ref.dense(h, cols), (V, F, which))
    same(dense_call(e, hip, hd, 1, h.astype(np.float32), P, eng.F32, VM, "device"), dot_ref.dense(h.astype(np.float32).astype(np.float64), ps), (V, "f32 vm"))
    hip.free_all()
    queries = {}
    for m in (0, 1, 255, 256, 257, 65536, 65537):
        ids = rng.choice(verts, size=m).astype(np.int32) if m else np.zeros(0, dtype=np.int32)  # (ids repeat: more entries than vertices)
        if m > 1:
            ids[m // 2] = ids[0]
        w = rng.standard_normal(m) * np.exp(3 * rng.standard_normal(m))
        off = np.array([0, m], dtype=np.int64)
        queries[m] = (ids, w)
        want = dot_ref.sparse(off, ids, w, ps)
        for src in ("host", "device"):
            same(sparse_call(e, hip, hd, 1, off, ids, w, src=src), want, (V, m, src))
        hip.free_all()
    order = (0, 1, 65537, 0, 257)
    off = np.concatenate([[0], np.cumsum(order)]).astype(np.int64)
    ids = np.concatenate([queries[m][0] for m in order]).astype(np.int32)
    w = np.concatenate([queries[m][1] for m in order])
    want = dot_ref.sparse(off, ids, w, rs)
    assert want[0, 0] == 0.0 and not np.signbit(want[0, 0])
    same(sparse_call(e, hip, hd, 1, off, ids, w, R, "host", "device"), want, (V, "mixed"))
    same(sparse_call(e, hip, hd, 1, off, ids, w, R, "device", "host"), want, (V, "mixed, device"))
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_vertices_without_a_row(hip):
    s = Marked(1, widths=(3, 10))
    V = s.V
    sp = s.e.id_space()
    assert sp["ids"] + sp["parked"] < V
    for hd, n in s.handles():
        ps, rs = cols_of(s.e, hd, n)
        absent = np.nonzero(np.all(np.stack(ps + rs, 1) == 0.0, axis=1))[0]
        assert len(absent) >= 2
        # a negative h on ids that never entered the stream: every term is -0.0 and so is their sum until the padding joins
        h = np.zeros((2, V))
        h[0, absent] = -1.0
        h[1, :] = -1.0
        want = dot_ref.dense(h, ps)
        same(dense_call(s.e, hip, hd, n, h), want, (hd, "negative h"))
        off = np.array([0, 2, 2 + len(absent)], dtype=np.int64)
        ids = np.concatenate([absent[:2], absent]).astype(np.int32)
        w = np.full(len(ids), -2.5)
        wsp = dot_ref.sparse(off, ids, w, ps)
        assert np.all(wsp == 0.0)
        same(sparse_call(s.e, hip, hd, n, off, ids, w), wsp, (hd, "sparse, absent ids"))
        # one-hot h: the point reads, bit for bit
        pick = np.concatenate([absent[:1], np.nonzero(ps[0] > 0)[0][:5], [0, V - 1]]).astype(np.int32)
        h = np.zeros((len(pick), V))
        h[np.arange(len(pick)), pick] = 1.0
        pa, ra = s.e.read_at(hd[1], pick) if hd[0] == "slot" else s.e.group_read_at(hd[1], pick)
        for which, at in ((P, pa), (R, ra)):
            got = dense_call(s.e, hip, hd, n, h, which)
            want = np.asarray(at).reshape(len(pick), n)
            assert np.array_equal(bits(np.abs(got)), bits(np.abs(want))), (hd, which)
            nz = want != 0.0
            assert np.array_equal(bits(got[nz]), bits(want[nz])), (hd, which)  # (a zero meets the padding: its sign is +)
            one = np.arange(len(pick) + 1, dtype=np.int64)
            same(sparse_call(s.e, hip, hd, n, one, pick, np.ones(len(pick)), which), got, (hd, which, "sparse one-hot"))
        hip.free_all()
    s.e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
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
    rng = np.random.default_rng(26)
    h = rng.standard_normal((3, V))
    off, ids, w = csr_of(h, 1.0)

    def check(what):
        for hd, n in handles:
            ps, rs = cols_of(e, hd, n)
            same(dense_call(e, hip, hd, n, h), dot_ref.dense(h, ps), (what, hd))
            same(dense_call(e, hip, hd, n, h, R, dest="device"), dot_ref.dense(h, rs), (what, hd, "r"))
            same(sparse_call(e, hip, hd, n, off, ids, w, src="device"), dot_ref.sparse(off, ids, w, ps), (what, hd, "sparse"))
        hip.free_all()

    check("before")
    for _ in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.update(slot, EPS)
        e.group_update(gid, EPS)
    sp = e.id_space()
    assert sp["renumberings"] > before["renumberings"] and sp["parked"] > 0 and sp["revivals"] > 0, (before, sp)
    check("after")
    # a parked vertex contributes its kept p: a one-hot h on a vertex that has left the window and still holds p > 0
    ps, _ = cols_of(e, ("group", gid), 10)
    in_window = np.zeros(V, dtype=bool)
    w1, w2 = g.window_edges()
    in_window[w1] = in_window[w2] = True
    gone = [(i, v) for i in range(10) for v in np.nonzero(~in_window & (ps[i] > 0))[0] if v >= 10]
    assert len(gone) > 0
    lane, v = gone[0]
    one = np.zeros((1, V))
    one[0, v] = 1.0
    got = dense_call(e, hip, ("group", gid), 10, one)
    assert got[0, lane] == ps[lane][v] > 0
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_churn_of_the_sources(hip):
    s = Marked(1, widths=(10, 3))
    e, gid, other = s.e, s.groups[10], s.groups[3]
    rng = np.random.default_rng(27)
    h = rng.standard_normal((5, s.V))
    off, ids, w = csr_of(h, 1.0)
    untouched = (dense_call(e, hip, ("group", other), 3, h), sparse_call(e, hip, ("group", other), 3, off, ids, w))
    idx, _ = e.group_add_source(gid, s.srcs[10])  # 10 -> 11
    assert idx == 10
    ps, _ = cols_of(e, ("group", gid), 11)
    got = dense_call(e, hip, ("group", gid), 11, h)
    assert got.shape == (5, 11)
    same(got, dot_ref.dense(h, ps), "after add")
    same(sparse_call(e, hip, ("group", gid), 11, off, ids, w, src="device", dest="device"), dot_ref.sparse(off, ids, w, ps), "after add, sparse")
    e.group_remove_source(gid, 0)
    ps, _ = cols_of(e, ("group", gid), 10)
    got = dense_call(e, hip, ("group", gid), 10, h, dest="device")
    assert got.shape == (5, 10)
    same(got, dot_ref.dense(h, ps), "after remove")
    same(sparse_call(e, hip, ("group", gid), 10, off, ids, w), dot_ref.sparse(off, ids, w, ps), "after remove, sparse")
    same(dense_call(e, hip, ("group", other), 3, h), untouched[0], "the other group, dense")
    same(sparse_call(e, hip, ("group", other), 3, off, ids, w), untouched[1], "the other group, sparse")
    e.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(hip):
    s = Marked(1, widths=(3,))
    e, gid, slot, n, V = s.e, s.groups[3], s.slot, 3, s.V
    L, hd = eng.lib(), e._h
    F = 2
    rng = np.random.default_rng(28)
    h = rng.standard_normal((F, V))
    d_h = put(hip, h)
    short_h = hip.alloc(8 * F * V - 8)
    out = np.full(F * n, 3.25)
    O = out.ctypes.data
    d_out, short_out = hip.alloc(8 * F * n), hip.alloc(8 * F * n - 8)
    off = np.array([0, 3, 5], dtype=np.int64)
    ids = np.array([1, 2, 2, 0, V - 1], dtype=np.int32)
    w = np.array([1.0, -2.0, 0.5, 4.0, 8.0])
    d_ids, d_w = put(hip, ids), put(hip, w)
    short_ids, short_w = hip.alloc(4 * 5 - 4), hip.alloc(8 * 5 - 8)
    H, D = eng.DEST_HOST, eng.DEST_DEVICE

    def untouched():
        return np.all(out == 3.25) and np.all(hip.read(d_out, 8 * F * n) == 0xAB) and np.all(hip.read(short_out, 8 * F * n - 8) == 0xAB)

    host_h = np.ascontiguousarray(h)
    bad_dense = [(gid, P, d_h, eng.F64, FM, 0, H, O), (gid, P, d_h, eng.F64, FM, eng.DOT_MAX_F + 1, H, O), (gid, P, d_h, eng.F64, FM, -1, H, O),
                 (gid, 2, d_h, eng.F64, FM, F, H, O), (gid, -1, d_h, eng.F64, FM, F, H, O), (gid, P, d_h, 2, FM, F, H, O), (gid, P, d_h, -1, FM, F, H, O),
                 (gid, P, d_h, eng.F64, 2, F, H, O), (gid, P, d_h, eng.F64, -1, F, H, O), (gid, P, d_h, eng.F64, FM, F, 2, O), (gid, P, d_h, eng.F64, FM, F, -1, O),
                 (gid, P, None, eng.F64, FM, F, H, O), (gid, P, d_h, eng.F64, FM, F, H, None), (gid, P, d_h, eng.F64, FM, F, D, None),
                 (7, P, d_h, eng.F64, FM, F, H, O), (-1, P, d_h, eng.F64, FM, F, H, O),
                 # a host pointer given as device memory; one element too short; misaligned
                 (gid, P, host_h.ctypes.data, eng.F64, FM, F, H, O), (gid, P, d_h, eng.F64, FM, F, D, O),
                 (gid, P, short_h, eng.F64, FM, F, H, O), (gid, P, short_h, eng.F64, VM, F, H, O), (gid, P, d_h, eng.F64, FM, F, D, short_out),
                 (gid, P, d_h + 4, eng.F32, FM, 2 * F, H, O),  # (aligned for f32, and one element too short)
                 (gid, P, d_h + 4, eng.F64, FM, F - 1, H, O), (gid, P, d_h + 2, eng.F32, FM, F, H, O), (gid, P, d_h, eng.F64, FM, F, D, d_out + 4)]
    for a in bad_dense:
        assert L.dppr_group_dot_dense_dev(hd, *a) == -1, a
        assert untouched(), a
    for a in [(3, P, d_h, eng.F64, FM, F, H, O), (slot, P, d_h, eng.F64, FM, 0, H, O), (slot, 2, d_h, eng.F64, FM, F, H, O), (slot, P, host_h.ctypes.data, eng.F64, FM, F, H, O),
              (slot, P, short_h, eng.F64, FM, F, H, O), (slot, P, d_h, eng.F64, FM, F, D, O), (slot, P, d_h, eng.F64, FM, F, D, d_out + 8 * F * n - 8)]:
        assert L.dppr_dot_dense_dev(hd, *a) == -1, a
        assert untouched(), a
    OFF = off.ctypes.data_as(I64P)
    I, Wp = ids.ctypes.data, w.ctypes.data
    dec = np.array([0, 3, 2], dtype=np.int64)
    first = np.array([1, 3, 5], dtype=np.int64)
    neg_id, big_id = ids.copy(), ids.copy()
    neg_id[1], big_id[4] = -1, V
    d_neg, d_big = put(hip, neg_id), put(hip, big_id)
    bad_sparse = [(gid, P, OFF, I, Wp, H, 0, H, O), (gid, P, OFF, I, Wp, H, eng.DOT_MAX_F + 1, H, O), (gid, 2, OFF, I, Wp, H, F, H, O),
                  (gid, P, OFF, I, Wp, 2, F, H, O), (gid, P, OFF, I, Wp, -1, F, H, O), (gid, P, OFF, I, Wp, H, F, 2, O),
                  (gid, P, None, I, Wp, H, F, H, O), (gid, P, OFF, None, Wp, H, F, H, O), (gid, P, OFF, I, None, H, F, H, O), (gid, P, OFF, I, Wp, H, F, H, None),
                  (gid, P, dec.ctypes.data_as(I64P), I, Wp, H, F, H, O), (gid, P, first.ctypes.data_as(I64P), I, Wp, H, F, H, O),
                  (7, P, OFF, I, Wp, H, F, H, O),
                  # host pointers given as device memory; one element too short; misaligned
                  (gid, P, OFF, I, d_w, D, F, H, O), (gid, P, OFF, d_ids, Wp, D, F, H, O), (gid, P, OFF, d_ids, d_w, D, F, D, O),
                  (gid, P, OFF, short_ids, d_w, D, F, H, O), (gid, P, OFF, d_ids, short_w, D, F, H, O), (gid, P, OFF, d_ids, d_w, D, F, D, short_out),
                  (gid, P, OFF, d_ids + 2, d_w, D, F, H, O), (gid, P, OFF, d_ids, d_w + 4, D, F, H, O), (gid, P, OFF, d_ids, d_w, D, F, D, d_out + 4),
                  # an id outside [0, V): from host memory (checked before any launch) and from device memory (the kernel's flag)
                  (gid, P, OFF, neg_id.ctypes.data, Wp, H, F, H, O), (gid, P, OFF, big_id.ctypes.data, Wp, H, F, H, O),
                  (gid, P, OFF, neg_id.ctypes.data, Wp, H, F, D, d_out), (gid, P, OFF, big_id.ctypes.data, Wp, H, F, D, d_out),
                  (gid, P, OFF, d_neg, d_w, D, F, H, O), (gid, P, OFF, d_big, d_w, D, F, H, O),
                  (gid, P, OFF, d_neg, d_w, D, F, D, d_out), (gid, P, OFF, d_big, d_w, D, F, D, d_out)]
    for a in bad_sparse:
        assert L.dppr_group_dot_sparse(hd, *a) == -1, a
        assert untouched(), a
    for a in [(3, P, OFF, I, Wp, H, F, H, O), (slot, P, OFF, I, Wp, H, 0, H, O), (slot, P, dec.ctypes.data_as(I64P), I, Wp, H, F, H, O),
              (slot, P, OFF, big_id.ctypes.data, Wp, H, F, H, O), (slot, P, OFF, d_big, d_w, D, F, D, d_out), (slot, P, OFF, d_neg, d_w, D, F, H, O)]:
        assert L.dppr_dot_sparse(hd, *a) == -1, a
        assert untouched(), a
    # the same buffers are good for the calls that fit them, and the engine answers
    ps, _ = cols_of(e, ("group", gid), n)
    assert L.dppr_group_dot_dense_dev(hd, gid, P, d_h, eng.F64, FM, F, D, d_out) == 0
    same(hip.read(d_out, 8 * F * n, np.float64).reshape(F, n), dot_ref.dense(h, ps), "valid dense after the rejections")
    assert L.dppr_group_dot_sparse(hd, gid, P, OFF, d_ids, d_w, D, F, H, O) == 0
    same(out.reshape(F, n), dot_ref.sparse(off, ids, w, ps), "valid sparse after the rejections")
    assert L.dppr_group_dot_dense_dev(hd, gid, P, short_h, eng.F32, FM, F, H, O) == 0  # (f32: the short buffer is long enough)
    e.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_bystanders_are_untouched(hip):
    s = Marked(1, widths=(10,))
    s.update(1)
    e, gid = s.e, s.groups[10]

    def snapshot():
        out = [x for k in (10, 8192) for t in e.group_topk(gid, k) for x in t]
        out += [np.asarray(x) for x in e.group_export_sparse(gid, 1e-6, with_r=True)]
        out += [x for i in range(10) for x in e.group_read(gid, i)]
        return out

    before = snapshot()
    rng = np.random.default_rng(29)
    h = rng.standard_normal((17, s.V))
    off, ids, w = csr_of(h, 1.0)
    for which in (P, R):
        dense_call(e, hip, ("group", gid), 10, h, which, dest="device")
        dense_call(e, hip, ("group", gid), 10, h.astype(np.float32), which, eng.F32, VM)
        sparse_call(e, hip, ("group", gid), 10, off, ids, w, which, "device", "device")
        sparse_call(e, hip, ("group", gid), 10, off, ids, w, which)
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
    rng = np.random.default_rng(30)
    h = rng.standard_normal((4, s.V))
    dense_call(s.e, hip, ("group", gid), 10, h)
    with_ws = eng.live_bytes()
    assert with_ws[0] > held[0] and with_ws[1] > held[1]  # the partials and the block, device and pinned
    dense_call(s.e, hip, ("group", gid), 10, h[:2], R)
    dense_call(s.e, hip, ("slot", s.slot), 1, h, dest="device")
    assert eng.live_bytes() == with_ws  # a smaller call takes nothing new
    off, ids, w = csr_of(h, 0.5)
    sparse_call(s.e, hip, ("group", gid), 10, off, ids, w)
    grown = eng.live_bytes()
    assert grown[0] > with_ws[0]  # the table, ids and weights of a host source
    sparse_call(s.e, hip, ("group", gid), 10, off, ids, w, src="device", dest="device")
    assert eng.live_bytes() == grown
    s.e.close()
    gc.collect()
    assert eng.live_bytes() == before
