"""The forward sweep (dppr_forward) on the device against the numpy restatement of tests/forward_ref.py over the rows the device
holds (dppr_read_graph + dppr_debug_id_map). f -- through the top k, the point reads and the dense copy --, rem and iters_used are
compared by bit pattern; the one tolerance in this file is the derived bound of the test that holds the forward sweep and the
reverse solves together."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import forward_ref as fr
from tests.test_export_gpu import Hip
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 5, 8, 10, 16)
ITERS = (1, 7, 8, 9, 64)
TOLS = (0.0, 1e-3, 1e-9)
EPS = 1e-9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rows_of(e, epoch=-1):
    row, col, _ = e.read_graph(epoch)
    return fr.Rows(e.V, row, col, e.id_map())


class Columns:
    """The reference columns of one set of rows, computed once per (start, iters, tol)."""

    def __init__(self, rows):
        self.rows, self.memo = rows, {}

    def __call__(self, q, iters, tol):
        key = (int(q), int(iters), float(tol))
        if key not in self.memo:
            self.memo[key] = fr.forward(self.rows, int(q), iters, tol)
        return self.memo[key]


def check_call(e, hip, cols, starts, iters, tol, what, k=40, min_f=0.0, at=None, dense=((eng.F64, eng.VERTEX_MAJOR),)):
    """One call with every part against the reference; returns the call's dict."""
    V, m = e.V, len(starts)
    at = np.arange(0, V, 7, dtype=np.int32) if at is None else at
    want = [cols(q, iters, tol) for q in starts]
    got = e.forward(starts, iters, tol, k=k, min_f=min_f, at=at)
    assert got["iters_used"].tolist() == [w[2] for w in want], (what, got["iters_used"], [w[2] for w in want])
    assert np.array_equal(bits(got["rem"]), bits([w[1] for w in want])), (what, got["rem"], [w[1] for w in want])
    for i, (f, _, _) in enumerate(want):
        ids, fk = fr.topk(f, k, min_f)
        assert np.array_equal(got["topk"][i][0], ids), (what, i, got["topk"][i][0][:8], ids[:8])
        assert np.array_equal(bits(got["topk"][i][1]), bits(fk)), (what, i)
        assert np.array_equal(bits(got["at"][i]), bits(f[at])), (what, i, "at")
    full = np.stack([w[0] for w in want])   # [m][V]
    for dtype, layout in dense:
        size = 4 if dtype == eng.F32 else 8
        ptr = hip.alloc(size * m * V + 16)
        e.forward(starts, iters, tol, dense_ptr=ptr, dtype=dtype, layout=layout)
        raw = hip.read(ptr, size * m * V + 16)
        assert np.all(raw[size * m * V:] == 0xAB), (what, "past the end")
        arr = raw[:size * m * V].view(np.float32 if dtype == eng.F32 else np.float64)
        arr = arr.reshape(m, V) if layout == eng.SOURCE_MAJOR else arr.reshape(V, m).T
        if dtype == eng.F32:
            assert np.array_equal(arr.view(np.uint32), full.astype(np.float32).view(np.uint32)), (what, "f32: the f64 result rounded once")
        else:
            assert np.array_equal(bits(arr), bits(full)), (what, "dense", layout)
    hip.free_all()
    return got


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_bit_for_bit_against_the_restatement(directed):
    """The R-MAT window at scale 10 with duplicate edges of tests/test_walks_gpu.py. Starts: the hub, a sink (directed), a vertex the
    stream never named, the hub again, three more, and repeats of all of them up to 16; every row width, every iteration count
    around a check, three tolerances."""
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    Wn, c = 4000, 50
    w1, w2 = e1[:Wn].astype(np.int64), e2[:Wn].astype(np.int64)
    assert len(np.unique(w1 * V + w2)) < Wn  # duplicate edges
    e = eng.Engine(V, Wn, directed, c)
    e.load_window(e1[:Wn], e2[:Wn])
    hip = Hip()
    rows = rows_of(e)
    cols = Columns(rows)
    x2i = e.id_map()
    hub = int(np.argmax(rows.d))
    unnamed = int(np.nonzero(x2i < 0)[0][0])
    sink = hub
    if directed:
        sinks = np.nonzero((rows.d == 0) & (np.diff(rows.ptr) > 0))[0]
        assert len(sinks)
        sink = int(sinks[0])
    r1, r2, r3 = (int(x) for x in np.nonzero((x2i >= 0) & (rows.d > 0))[0][[5, 50, 200]])
    starts = np.array([hub, sink, unnamed, hub, r1, r2, r3, sink, r1, hub, unnamed, r2, r3, r1, hub, sink], dtype=np.int32)
    assert np.diff(rows.ptr).max() > 64   # an in-row longer than a wave
    frozen_early = running = 0
    for m in WIDTHS:
        for iters in ITERS:
            for tol in TOLS:
                dense = ((eng.F64, eng.VERTEX_MAJOR), (eng.F32, eng.SOURCE_MAJOR)) if iters == 64 else ((eng.F64, eng.SOURCE_MAJOR),)
                if iters in (1, 8) and tol:
                    dense = ()
                got = check_call(e, hip, cols, starts[:m], iters, tol, (directed, m, iters, tol), dense=dense)
                frozen_early += int(np.sum(got["iters_used"] < iters))
                running += int(np.sum(got["iters_used"] == iters))
    assert frozen_early > 0 and running > 0
    # the unnamed start and the sink: f = 0.15 e_q, nothing remains, stopped at the first check
    f, rem, used = cols(unnamed, 64, 0.0)
    assert used == 8 and rem == 0.0 and f[unnamed] == 0.15 and np.count_nonzero(f) == 1
    if directed:
        f, rem, used = cols(sink, 64, 0.0)
        assert used == 8 and rem == 0.0 and np.count_nonzero(f) == 1
    # the hub's column does not die, and 1e-3 stops it before 1e-9 does
    assert cols(hub, 64, 0.0)[2] == 64 and cols(hub, 64, 1e-3)[2] < cols(hub, 64, 1e-9)[2] <= 64
    # a top k beyond what qualifies, a threshold that cuts, the whole vector
    check_call(e, hip, cols, starts[:5], 64, 1e-9, "k = 8192", k=8192)
    check_call(e, hip, cols, starts[:5], 64, 1e-9, "min_f", k=100, min_f=1e-4)
    check_call(e, hip, cols, starts[:5], 64, 1e-9, "min_f above 0.15", k=3, min_f=0.2)
    check_call(e, hip, cols, starts[:3], 9, 0.0, "every id", at=np.arange(V, dtype=np.int32)[::-1].copy())
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def star(D):
    """ONE head (vertex 0) of in-degree D: tails 1 .. D, each with (i % 5) further out-edges so that their terms differ; a start S
    that feeds every tail; the head feeds S back, so the mass keeps moving. Returns (V, tails, heads, S)."""
    S, first_sink = D + 1, D + 2
    t = [np.arange(1, D + 1), np.full(D, S), [0]]
    h = [np.zeros(D, dtype=np.int64), np.arange(1, D + 1), [S]]
    for extra in range(1, 5):
        who = np.arange(1, D + 1)[np.arange(1, D + 1) % 5 >= extra]
        t.append(who)
        h.append(np.full(len(who), first_sink + extra))
    return first_sink + 5, np.concatenate(t).astype(np.int32), np.concatenate(h).astype(np.int32), S


@pytest.mark.parametrize("D", [63, 64, 65, 4097, 65537])
def test_fold_boundaries(D):
    """An in-row of exactly D entries -- below, at and above a wave's worth, above a piece of 4096, across the block of 2^16 -- at
    every piece size and every team width: the bits of the restatement, whatever the setting."""
    V, tails, heads, S = star(D)
    order = np.random.default_rng(D).permutation(len(tails))   # internal ids are not the star's order
    e = eng.Engine(V, len(tails), 1, 1)
    e.load_window(tails[order], heads[order])
    hip = Hip()
    rows = rows_of(e)
    assert np.diff(rows.ptr)[0] == D and np.diff(rows.ptr).max() == D
    cols = Columns(rows)
    at = np.array([0, 1, 2, D, S], dtype=np.int32)
    first = {}
    for m, starts in ((3, [S, 2, 0]), (16, [S, 0, 5] + [S] * 13)):
        starts = np.array(starts, dtype=np.int32)
        for piece in (0, 64, 4096):
            for team in (0, 1, 2, 4, 8):
                e.debug_forward(piece, team)
                got = check_call(e, hip, cols, starts, 9, 0.0, (D, m, piece, team), k=8, at=at, dense=())
                key = (m,)
                blob = b"".join(np.asarray(x).tobytes() for x in (got["rem"], got["at"]) + tuple(got["topk"][0]))
                assert first.setdefault(key, blob) == blob, (D, m, piece, team)
    # the head's sum is the fold's, not the running sum's (the comparison above can fail)
    f, _, _ = cols(S, 9, 0.0)
    assert f[0] > 0.0
    if D >= 4097:
        y = (fr.DAMP * (fr.DAMP / (D + 1.0))) / (rows.d[rows.tails[rows.ptr[0]:rows.ptr[1]]] + 1.0)
        from tests import dot_ref
        assert dot_ref.fold(y) != dot_ref.running(y)
    e.debug_forward(0, 0)
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_independence_and_determinism():
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    e = eng.Engine(V, 4000, 1, 50)
    e.load_window(e1[:4000], e2[:4000])
    rows = rows_of(e)
    named = np.nonzero((e.id_map() >= 0) & (rows.d > 0))[0]
    starts = named[np.random.default_rng(5).permutation(len(named))[:16]].astype(np.int32)
    starts[3] = np.nonzero((e.id_map() >= 0) & (rows.d == 0))[0][0]   # a sink: its column dies at the first check
    starts[11] = np.nonzero(e.id_map() < 0)[0][0]
    at = np.arange(V, dtype=np.int32)
    together = e.forward(starts, 64, 1e-3, k=50, at=at)
    used = together["iters_used"]
    assert len(set(used.tolist())) > 1, used   # mixed freezing: the columns stop at different checks
    for i in (0, 7, 15):
        alone = e.forward(starts[i:i + 1], 64, 1e-3, k=50, at=at)
        assert alone["iters_used"][0] == used[i] and bits(alone["rem"])[0] == bits(together["rem"])[i]
        assert np.array_equal(bits(alone["at"][0]), bits(together["at"][i]))
        assert np.array_equal(alone["topk"][0][0], together["topk"][i][0])
    again = e.forward(starts, 64, 1e-3, k=50, at=at)
    for k in ("iters_used", "rem", "at"):
        assert np.asarray(again[k]).tobytes() == np.asarray(together[k]).tobytes(), k
    # another position in the call, another width: the same column
    rev = e.forward(starts[::-1].copy()[:5], 64, 1e-3, at=at)
    assert np.array_equal(bits(rev["at"][0]), bits(together["at"][15]))
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_two_directions_agree():
    """p_i[q] of a converged reverse solve and f_q[s_i] of the forward sweep are the same entry of the PPR matrix:
    |f_q[s_i] - p_i[q]| <= eps + rem_q + 1e-12 -- eps bounds |p - pihat|inf through the certificate, rem the truncation, 1e-12 the
    rounding of <= 256 sums of values <= 1. For a set lane h the same bound times sum(h)."""
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    Wn = 4000
    e = eng.Engine(V, Wn, 1, 50)
    e.load_window(e1[:Wn], e2[:Wn])
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, Wn, 1, 10)]
    gid = e.add_source_group(srcs)
    e.group_init_solve(gid, EPS)
    named = np.nonzero(e.id_map() >= 0)[0]
    rng = np.random.default_rng(17)
    sets = [(np.sort(rng.choice(named, 40, replace=False)).astype(np.int32), rng.random(40) + 0.1) for _ in range(2)]
    tg = e.add_target_group(sets)
    e.group_init_solve(tg, EPS)
    cert = e.group_certify(gid, EPS)
    assert np.all(cert["max_abs_r"] <= EPS) and np.all(cert["n_pos"] == 0) and np.all(cert["n_neg"] == 0)
    q = rng.choice(named, 16, replace=False).astype(np.int32)
    got = e.forward(q, 256, 0.0, at=np.arange(V, dtype=np.int32))
    f, rem = got["at"], got["rem"]
    assert np.all(rem >= 0.0) and np.all(rem < 1e-9)
    worst = 0.0
    for i, s in enumerate(srcs):
        p, _ = e.group_read(gid, i)
        gap = np.abs(f[:, s] - p[q])
        worst = max(worst, float(np.max(gap - rem)))
        assert np.all(gap <= EPS + rem + 1e-12), (i, gap.max())
    for i, (ids, w) in enumerate(sets):
        p, _ = e.group_read(tg, i)
        gap = np.abs(f[:, ids] @ w - p[q])
        assert np.all(gap <= (EPS + rem + 1e-12) * w.sum()), (i, gap.max())
    print("largest |f_q[s] - p_s[q]| - rem:", worst)
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def group_blob(e, gid, n):
    return b"".join(x.tobytes() for i in range(n) for x in e.group_read(gid, i))


def test_across_the_stream():
    """After slides, after a renumbering and on a parked start the result is the restatement over the rows then held; an epoch that
    is not resident is refused; the states of a bystander group are not touched."""
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c, n_epochs=2)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    gid = e.add_source_group([0, 1, 2])
    e.group_init_solve(gid, EPS)
    e.group_mark(gid)
    hip = Hip()
    newest, seen_renumberings = 0, 0
    for b in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        newest = e.slide(*g.new_stream())
        e.group_update(gid, EPS)
        sp = e.id_space()
        if b in (0, 1, batches - 1) or sp["renumberings"] > seen_renumberings:
            seen_renumberings = sp["renumberings"]
            before = group_blob(e, gid, 3)
            rows = rows_of(e)
            named = np.nonzero((e.id_map() >= 0) & (rows.d > 0))[0]
            starts = np.array([named[0], named[len(named) // 2], named[-1], 0, 1], dtype=np.int32)
            check_call(e, hip, Columns(rows), starts, 24, 1e-6, ("batch", b), dense=())
            assert group_blob(e, gid, 3) == before
    sp = e.id_space()
    assert sp["parked"] > 0 and sp["renumberings"] > 0, sp
    id_map = e.id_map()
    parked = np.nonzero(id_map >= V - sp["parked"])[0]
    unnamed = np.nonzero(id_map < 0)[0]
    assert len(parked) and len(unnamed)
    rows = rows_of(e)
    cols = Columns(rows)
    starts = np.array([parked[0], unnamed[0], int(np.argmax(rows.d)), parked[-1]], dtype=np.int32)
    before = group_blob(e, gid, 3)
    changes_before = [np.asarray(x).tobytes() for t in e.group_changes(gid, 50) for x in t]
    got = check_call(e, hip, cols, starts, 64, 1e-9, "parked", at=np.concatenate([starts, parked[:5], unnamed[:5]]).astype(np.int32),
                     dense=((eng.F64, eng.VERTEX_MAJOR), (eng.F32, eng.SOURCE_MAJOR)))
    assert got["iters_used"][0] == 8 and got["rem"][0] == 0.0 and got["iters_used"][1] == 8
    assert got["topk"][0][0].tolist() == [parked[0]] and got["topk"][0][1].tolist() == [0.15]
    assert got["topk"][1][0].tolist() == [unnamed[0]] and got["topk"][1][1].tolist() == [0.15]
    assert group_blob(e, gid, 3) == before
    assert [np.asarray(x).tobytes() for t in e.group_changes(gid, 50) for x in t] == changes_before   # the mark stands
    # the older resident epoch: accepted unless a renumbering came between; one that left the ring: refused
    with pytest.raises(eng.DpprError, match="not resident"):
        e.forward(starts, 8, epoch=newest - 2)
    with pytest.raises(eng.DpprError, match="not resident"):
        e.forward(starts, 8, epoch=newest + 1)
    e.close()


def test_rejections_write_nothing():
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    e = eng.Engine(V, 4000, 1, 50)
    e.load_window(e1[:4000], e2[:4000])
    hip = Hip()
    L, h = e._L, e._h
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ints, dbls = np.full(64, 77, dtype=np.int32), np.full(64, 7.5)
    d_dense = hip.alloc(8 * 2 * V)
    good = np.array([1, 2], dtype=np.int32)

    def out(**kw):
        o = eng.ForwardOut()
        o.iters_used, o.rem = ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp)
        o.k, o.min_f = 4, 0.0
        o.topk_ids, o.topk_f, o.topk_counts = ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp), ints.ctypes.data_as(ip)
        o.at_ids, o.n_at, o.at_f = good.ctypes.data_as(ip), 2, dbls.ctypes.data_as(dp)
        o.dense_dev, o.dense_dtype, o.dense_layout = d_dense, eng.F64, eng.VERTEX_MAJOR
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def refused(starts=good, m=2, iters=8, tol=0.0, epoch=-1, o=None, **kw):
        o = out(**kw) if o is None else o
        sp = None if starts is None else starts.ctypes.data_as(ip)
        rc = L.dppr_forward(h, epoch, sp, m, iters, tol, None if o == "null" else C.byref(o))
        clean = np.all(ints == 77) and np.all(dbls == 7.5) and np.all(hip.read(d_dense, 8 * 2 * V) == 0xAB)
        return rc == -1 and bool(clean)

    bad_id, neg_id = np.array([1, V], dtype=np.int32), np.array([-1, 2], dtype=np.int32)
    for kw in (dict(m=0), dict(m=17), dict(m=-1), dict(iters=0), dict(iters=257), dict(tol=-1e-300), dict(tol=float("nan")),
               dict(tol=float("inf")), dict(starts=None), dict(o="null"), dict(starts=bad_id), dict(starts=neg_id), dict(epoch=1),
               dict(epoch=7), dict(k=0), dict(k=8193), dict(min_f=-1.0), dict(min_f=float("nan")), dict(topk_ids=None),
               dict(topk_counts=None), dict(at_ids=None), dict(at_f=None), dict(n_at=0), dict(n_at=4097),
               dict(at_ids=bad_id.ctypes.data_as(ip)), dict(dense_dtype=2), dict(dense_layout=-1), dict(dense_dev=d_dense + 4),
               dict(dense_dev=d_dense + 8), dict(dense_dev=ints.ctypes.data)):
        assert refused(**kw), list(kw)
    assert L.dppr_forward(None, -1, good.ctypes.data_as(ip), 2, 8, 0.0, C.byref(out())) == -1
    for bad in ((32, 0), (96, 0), (8192, 0), (-1, 0), (0, 3), (0, 16), (0, -1)):
        with pytest.raises(eng.DpprError):
            e.debug_forward(*bad)
    # a call that asks for nothing runs nothing; a part whose pointers are all NULL is not run
    assert L.dppr_forward(h, -1, good.ctypes.data_as(ip), 2, 8, 0.0, C.byref(eng.ForwardOut())) == 0
    only = eng.ForwardOut()
    only.rem = dbls.ctypes.data_as(dp)
    assert L.dppr_forward(h, -1, good.ctypes.data_as(ip), 2, 8, 0.0, C.byref(only)) == 0
    assert np.all(dbls[:2] != 7.5) and np.all(dbls[2:] == 7.5) and np.all(ints == 77) and np.all(hip.read(d_dense, 8 * 2 * V) == 0xAB)
    hip.free_all()
    e.close()


def test_every_buffer_goes_with_the_engine():
    gc.collect()
    before = eng.live_bytes()
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    e = eng.Engine(V, 4000, 1, 50)
    e.load_window(e1[:4000], e2[:4000])
    held = eng.live_bytes()
    e.set_profiling(1)
    got = e.forward([1, 2, 3], 16, k=5)
    assert len(got["topk"]) == 3 and e.query_ms() > 0.0
    assert eng.live_bytes()[0] > held[0] and eng.live_bytes()[1] > held[1]
    e.close()
    assert eng.live_bytes() == before
