"""The forward push (dppr_forward_push) on the device against the numpy restatement of tests/fpush_ref.py over the rows the device
holds (dppr_read_graph + dppr_debug_id_map). p and r -- through the top k, the point reads and the dense copies --, rem, the
per-column statistics and `work` are compared by bit pattern or as integers; the tolerances in this file are the derived bounds
of the entrywise guarantee and of the bidirectional estimate."""
import ctypes as C

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import forward_ref as fr
from tests import fpush_ref as pr
from tests.test_export_gpu import Hip
from tests.test_forward_gpu import bits, rows_of, star
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 5, 8, 10, 16)
EPSS = (1e-4, 1e-6, 1e-8)
ROUNDS = (1, 8, 64)
# rounds the hub's column takes on the R-MAT window (a CPU run of the definition): converged within 64, never within 8
HUB_ROUNDS = {(1, 1e-4): 10, (1, 1e-6): 26, (1, 1e-8): 41, (0, 1e-4): 11, (0, 1e-6): 32, (0, 1e-8): 52}


def as_set(s):
    if np.isscalar(s):
        return np.array([s], dtype=np.int64), np.ones(1)
    return np.asarray(s[0], dtype=np.int64), np.asarray(s[1], dtype=np.float64)


class Columns:
    """The reference columns of one set of rows, computed once per (set, eps, max_rounds) and never changed."""

    def __init__(self, e, rows=None):
        self.rows = rows_of(e) if rows is None else rows
        self.rowless = pr.rowless_mask(self.rows)
        self.memo = {}

    def __call__(self, s, eps, max_rounds):
        ids, w = as_set(s)
        key = (ids.tobytes(), w.tobytes(), float(eps), int(max_rounds))
        if key not in self.memo:
            self.memo[key] = pr.push(self.rows, self.rowless, ids, w, eps, max_rounds)
        return self.memo[key]


def check_call(e, hip, cols, sets, eps, max_rounds, what, k=40, min_p=0.0, at=None, dense=((eng.F64, eng.VERTEX_MAJOR),)):
    """One call with every part against the reference; returns (the call's dict, the reference columns)."""
    V, m = e.V, len(sets)
    at = np.arange(0, V, 7, dtype=np.int32) if at is None else at
    want = [cols(s, eps, max_rounds) for s in sets]
    got = e.forward_push(sets, eps, max_rounds, k=k, min_p=min_p, at=at)
    for key in ("rounds_used", "converged", "pushes", "left"):
        assert got[key].tolist() == [getattr(w, key) for w in want], (what, key, got[key], [getattr(w, key) for w in want])
    assert np.array_equal(bits(got["rem"]), bits([w.rem for w in want])), (what, got["rem"], [w.rem for w in want])
    assert got["work"].tolist() == pr.work(cols.rows, want).tolist(), (what, got["work"], pr.work(cols.rows, want))
    for i, w in enumerate(want):
        ids, pk = fr.topk(w.p, k, min_p)
        assert np.array_equal(got["topk"][i][0], ids), (what, i, got["topk"][i][0][:8], ids[:8])
        assert np.array_equal(bits(got["topk"][i][1]), bits(pk)), (what, i)
        assert np.array_equal(bits(got["at_p"][i]), bits(w.p[at])), (what, i, "at_p")
        assert np.array_equal(bits(got["at_r"][i]), bits(w.r[at])), (what, i, "at_r")
    full = {"p": np.stack([w.p for w in want]), "r": np.stack([w.r for w in want])}   # [m][V]
    for dtype, layout in dense:
        size = 4 if dtype == eng.F32 else 8
        ptr = {"p": hip.alloc(size * m * V + 16), "r": hip.alloc(size * m * V + 16)}
        e.forward_push(sets, eps, max_rounds, dense_p_ptr=ptr["p"], dense_r_ptr=ptr["r"], dtype=dtype, layout=layout)
        for name in ("p", "r"):
            raw = hip.read(ptr[name], size * m * V + 16)
            assert np.all(raw[size * m * V:] == 0xAB), (what, name, "past the end")
            arr = raw[:size * m * V].view(np.float32 if dtype == eng.F32 else np.float64)
            arr = arr.reshape(m, V) if layout == eng.SOURCE_MAJOR else arr.reshape(V, m).T
            if dtype == eng.F32:
                assert np.array_equal(arr.view(np.uint32), full[name].astype(np.float32).view(np.uint32)), (what, name, "f32: rounded once")
            else:
                assert np.array_equal(bits(arr), bits(full[name])), (what, name, "dense", layout)
        hip.free_all()
    return got, want


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_bit_for_bit_against_the_restatement(directed):
    """The R-MAT window at scale 10 of tests/test_forward_gpu.py. Columns: the hub, a sink, a vertex the stream never named, a
    two-seed set of the hub and a low-degree vertex (weights 0.25 and 3.0), a 64-seed set with an unnamed id in it, and repeats up
    to 16; every row width, three eps, three caps on the rounds."""
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    Wn, c = 4000, 50
    e = eng.Engine(V, Wn, directed, c)
    e.load_window(e1[:Wn], e2[:Wn])
    hip = Hip()
    cols = Columns(e)
    rows, x2i = cols.rows, e.id_map()
    hub = int(np.argmax(rows.d))
    unnamed = int(np.nonzero(x2i < 0)[0][0])
    sink = hub
    if directed:
        sinks = np.nonzero((rows.d == 0) & (np.diff(rows.ptr) > 0))[0]
        assert len(sinks)
        sink = int(sinks[0])
    low = int(np.nonzero((x2i >= 0) & (rows.d == 1))[0][3])
    named = np.nonzero(x2i >= 0)[0]
    rng = np.random.default_rng(11)
    big_ids = np.concatenate([rng.choice(named, 63, replace=False), [unnamed]])
    big = (big_ids[rng.permutation(64)], rng.random(64) + 0.05)
    two = (np.array([hub, low]), np.array([0.25, 3.0]))
    r1 = int(np.nonzero((x2i >= 0) & (rows.d > 0))[0][50])
    sets = [hub, sink, unnamed, two, big, r1, hub, big, sink, two, unnamed, r1, hub, two, big, sink]
    assert np.diff(rows.ptr).max() > 64   # an in-row longer than a wave
    early = capped = 0
    for m in WIDTHS:
        for eps in EPSS:
            for max_rounds in ROUNDS:
                dense = ((eng.F64, eng.VERTEX_MAJOR), (eng.F32, eng.SOURCE_MAJOR)) if max_rounds == 64 else ((eng.F64, eng.SOURCE_MAJOR),)
                if max_rounds == 1 and eps != 1e-6:
                    dense = ()
                got, want = check_call(e, hip, cols, sets[:m], eps, max_rounds, (directed, m, eps, max_rounds), dense=dense)
                early += int(np.sum((got["converged"] == 1) & (got["rounds_used"] < max_rounds)))
                capped += int(np.sum(got["converged"] == 0))
    assert early > 0 and capped > 0   # some columns converge early, some hit the cap
    for eps in EPSS:
        h64, h8 = cols(hub, eps, 64), cols(hub, eps, 8)
        print("hub rounds", directed, eps, h64.rounds_used)
        assert h64.converged == 1 and h64.rounds_used == HUB_ROUNDS[(directed, eps)] and h8.converged == 0 and h8.rounds_used == 8
        assert min(pr.gathered_per_round(rows, h64)) < int(np.sum(np.diff(rows.ptr) > 0))   # a round gathers fewer rows than the window has
    # the unnamed start: settled exactly, no round, no statistic
    u = cols(unnamed, 1e-6, 64)
    assert u.rounds_used == 0 and u.converged == 1 and u.pushes == 0 and u.rem == 0.0 and u.p[unnamed] == 0.15 and np.count_nonzero(u.p) == 1
    # a top k beyond what qualifies, a threshold that cuts (the unnamed seed of the 64-seed set stands in its place), every id
    check_call(e, hip, cols, sets[:5], 1e-6, 64, "k = 8192", k=8192)
    check_call(e, hip, cols, sets[:5], 1e-6, 64, "min_p", k=100, min_p=1e-3)
    check_call(e, hip, cols, sets[:5], 1e-6, 64, "k = 3", k=3, min_p=0.02)
    check_call(e, hip, cols, sets[:3], 1e-8, 9, "every id", at=np.arange(V, dtype=np.int32)[::-1].copy())
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5000, 65537])
def test_long_rows(D):
    """The star of tests/test_forward_gpu.py: ONE head of in-degree D whose tails the start S feeds, so the head's row is gathered
    in pieces, with most terms +0.0 in the later rounds (fewer tails stay above thr each time). D = 5000 under piece_edges = 64 and
    every other debug setting, D just above 2^16 across the block of the fold: the bits of the default setting and of numpy."""
    V, tails, heads, S = star(D)
    order = np.random.default_rng(D).permutation(len(tails))   # internal ids are not the star's order
    e = eng.Engine(V, len(tails), 1, 1)
    e.load_window(tails[order], heads[order])
    hip = Hip()
    cols = Columns(e)
    assert np.diff(cols.rows.ptr)[0] == D
    at = np.array([0, 1, 2, 3, 4, 5, D, S], dtype=np.int32)
    sets = [S, (np.array([S, 3]), np.array([2.0, 0.5])), 0]
    eps, max_rounds = (4e-6, 12) if D == 5000 else (3e-7, 7)
    settings = [(p, t, c) for p in (0, 64, 4096) for t in (0, 1, 8) for c in (0, 1, 5)] if D == 5000 else [(0, 0, 0), (64, 2, 3)]
    first = None
    for piece, team, chunk in settings:
        e.debug_forward_push(piece, team, chunk)
        got, want = check_call(e, hip, cols, sets, eps, max_rounds, (D, piece, team, chunk), k=8, at=at,
                               dense=((eng.F64, eng.SOURCE_MAJOR),) if (piece, team, chunk) in ((0, 0, 0), (64, 2, 3)) else ())
        blob = b"".join(np.asarray(got[x]).tobytes() for x in ("rem", "at_p", "at_r", "work", "pushes", "left", "rounds_used"))
        first = blob if first is None else first
        assert blob == first, (D, piece, team, chunk)
    # the head is gathered more than once, and in a later round only a part of its tails is in the frontier
    w = cols(S, eps, max_rounds)
    into_head = [int(F[1:D + 1].sum()) for F in w.fronts]
    assert sum(1 for n in into_head if n > 0) >= 2 and 0 < min(n for n in into_head if n > 0) < D, into_head
    e.debug_forward_push(0, 0, 0)
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_column_alone_and_among_fifteen_others():
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    e = eng.Engine(V, 4000, 1, 50)
    e.load_window(e1[:4000], e2[:4000])
    rows = rows_of(e)
    named = np.nonzero((e.id_map() >= 0) & (rows.d > 0))[0]
    rng = np.random.default_rng(5)
    starts = named[rng.permutation(len(named))[:16]]
    sets = [int(q) for q in starts]
    sets[7] = (starts[:9].copy(), rng.random(9) + 0.1)
    at = np.arange(V, dtype=np.int32)
    together = e.forward_push(sets, 1e-4, 10, k=50, at=at)
    assert len(set(together["rounds_used"].tolist())) > 1 and 0 < together["converged"].sum() < 16, together
    for i in (0, 7, 15):
        alone = e.forward_push(sets[i:i + 1], 1e-4, 10, k=50, at=at)
        for key in ("rounds_used", "converged", "pushes", "left"):
            assert alone[key][0] == together[key][i], (i, key)
        assert bits(alone["rem"])[0] == bits(together["rem"])[i]
        assert np.array_equal(bits(alone["at_p"][0]), bits(together["at_p"][i])) and np.array_equal(bits(alone["at_r"][0]), bits(together["at_r"][i]))
        assert np.array_equal(alone["topk"][0][0], together["topk"][i][0])
    again = e.forward_push(sets, 1e-4, 10, k=50, at=at)
    for key in ("rounds_used", "converged", "pushes", "left", "rem", "work", "at_p", "at_r"):
        assert np.asarray(again[key]).tobytes() == np.asarray(together[key]).tobytes(), key
    rev = e.forward_push(sets[::-1][:5], 1e-4, 10, at=at)   # another position in the call, another width: the same column
    assert np.array_equal(bits(rev["at_p"][0]), bits(together["at_p"][15])) and np.array_equal(bits(rev["at_r"][0]), bits(together["at_r"][15]))
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_entrywise_bound():
    """0 <= pihat_h - p <= rem entrywise on a graph small enough for a dense solve; the slack 1e-13 covers the rounding of the
    solve and of at most 64 rounds of sums of values <= sum(h) <= 4."""
    V, E = 300, 1500
    rng = np.random.default_rng(3)
    tails, heads = rng.integers(0, V, E).astype(np.int32), rng.integers(0, V, E).astype(np.int32)
    e = eng.Engine(V, E, 1, 1)
    e.load_window(tails, heads)
    rows = rows_of(e)
    stored = (rows.tails, rows.heads)
    x2i = e.id_map()
    named = np.nonzero(x2i >= 0)[0]
    sets = [int(named[0]), int(named[17]), (named[[5, 40, 99]], np.array([0.5, 2.0, 1.5])), (named[::4], rng.random(len(named[::4])) * 0.05 + 0.001)]
    at = np.arange(V, dtype=np.int32)
    seen = set()
    for eps, max_rounds in ((1e-3, 64), (1e-5, 64), (1e-7, 3), (1e-9, 64)):
        got = e.forward_push(sets, eps, max_rounds, at=at)
        thr = eps * (rows.d + 1.0)
        for i, s in enumerate(sets):
            ids, w = as_set(s)
            exact = sum(wq * fr.exact(V, stored[0], stored[1], int(q)) for q, wq in zip(ids, w))
            p, r, rem = got["at_p"][i], got["at_r"][i], got["rem"][i]
            gap = exact - p
            print("fpush bound", eps, max_rounds, i, "min gap", gap.min(), "max gap - rem", (gap - rem).max(), "rem", rem)
            assert np.all(gap >= -1e-13) and np.all(gap <= rem + 1e-13), (eps, i)
            assert np.all(r >= 0.0) and (got["left"][i] == 0) == bool(got["converged"][i]) and got["left"][i] == np.sum(r > thr)
            if got["converged"][i]:
                assert np.all(r <= thr)
            seen.add(int(got["converged"][i]))
    assert seen == {0, 1}
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_bidirectional_estimate():
    """pihat_h(s) = p_f[s] + sum_u r_f[u] pihat_u(s) exactly. A group solved at EPS holds p_i[u] with |p_i[u] - pihat_u(s_i)| <= EPS,
    so the dot of r_f with it is off by at most rem * EPS; f_256 of dppr_forward is below pihat by at most rem_256; 1e-12 covers
    the rounding of the sums: |p_f[s_i] + group_dot(r_f)[i] - f_256[s_i]| <= rem * EPS + rem_256 + 1e-12. Derived, not tuned."""
    EPS = 1e-9
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    Wn = 4000
    e = eng.Engine(V, Wn, 1, 50)
    e.load_window(e1[:Wn], e2[:Wn])
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, Wn, 1, 10)]
    gid = e.add_source_group(srcs)
    e.group_init_solve(gid, EPS)
    rows = rows_of(e)
    named = np.nonzero((e.id_map() >= 0) & (rows.d > 0))[0]
    q = np.random.default_rng(17).choice(named, 8, replace=False).astype(np.int32)
    m = len(q)
    hip = Hip()
    f = e.forward(q, 256, 0.0, at=np.array(srcs, dtype=np.int32))
    f256, rem256 = f["at"], f["rem"]   # [m][10], [m]
    for eps in (1e-4, 1e-6):
        d_r = hip.alloc(8 * m * V)
        got = e.forward_push([int(x) for x in q], eps, 64, at=np.array(srcs, dtype=np.int32), dense_r_ptr=d_r, dtype=eng.F64, layout=eng.SOURCE_MAJOR)
        dot = e.group_dot_dense_dev(gid, d_r, m)   # [m][10]
        est = got["at_p"] + dot
        gap = np.abs(est - f256)
        bound = (got["rem"] * EPS + rem256 + 1e-12)[:, None]
        print("fpush bidirectional", eps, "largest gap", gap.max(), "smallest bound", bound.min(), "rem", got["rem"].max())
        assert np.all(gap <= bound), (eps, gap.max())
        assert np.all(got["rem"] > 0.0)
    hip.free_all()
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_after_a_renumbering():
    """After slides and a renumbering, with parked and unnamed seeds in a set: the restatement over the rows then held."""
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c, n_epochs=2)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    gid = e.add_source_group([0, 1, 2])   # (a solver that follows the stream: renumberings happen between its updates)
    e.group_init_solve(gid, 1e-9)
    hip = Hip()
    newest = 0
    for b in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        newest = e.slide(*g.new_stream())
        e.group_update(gid, 1e-9)
    before = b"".join(x.tobytes() for i in range(3) for x in e.group_read(gid, i))
    sp = e.id_space()
    assert sp["parked"] > 0 and sp["renumberings"] > 0, sp
    id_map = e.id_map()
    parked = np.nonzero(id_map >= V - sp["parked"])[0]
    unnamed = np.nonzero(id_map < 0)[0]
    cols = Columns(e)
    named = np.nonzero((id_map >= 0) & (cols.rows.d > 0))[0]
    mixed = (np.array([named[3], parked[0], unnamed[0], named[-1]]), np.array([1.0, 0.7, 0.2, 2.0]))
    sets = [int(named[0]), int(parked[0]), mixed, int(np.argmax(cols.rows.d)), int(unnamed[0])]
    at = np.concatenate([np.arange(0, V, 5), parked[:5], unnamed[:5]]).astype(np.int32)
    got, want = check_call(e, hip, cols, sets, 1e-6, 24, "renumbered", at=at, dense=((eng.F64, eng.VERTEX_MAJOR), (eng.F32, eng.SOURCE_MAJOR)))
    assert got["rounds_used"][1] == 0 and got["pushes"][1] == 0 and got["rem"][1] == 0.0
    assert got["topk"][1][0].tolist() == [parked[0]] and got["topk"][1][1].tolist() == [0.15]
    assert got["topk"][4][0].tolist() == [unnamed[0]]
    assert want[2].p[parked[0]] == 0.15 * 0.7 and want[2].p[unnamed[0]] == 0.15 * 0.2
    assert b"".join(x.tobytes() for i in range(3) for x in e.group_read(gid, i)) == before   # no state is changed
    with pytest.raises(eng.DpprError, match="not resident"):
        e.forward_push(sets, 1e-6, 8, epoch=newest - 2)
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing():
    V, e1, e2 = datagen.rmat_stream(10, 20000, 7)
    e = eng.Engine(V, 4000, 1, 50)
    e.load_window(e1[:4000], e2[:4000])
    hip = Hip()
    L, h = e._L, e._h
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    ints, dbls, longs = np.full(64, 77, dtype=np.int32), np.full(64, 7.5), np.full(64, 77, dtype=np.int64)
    d_p, d_r = hip.alloc(8 * 2 * V), hip.alloc(8 * 2 * V)
    at_ids = np.array([1, 2], dtype=np.int32)
    good = (np.array([0, 1, 3], dtype=np.int64), np.array([1, 2, 5], dtype=np.int32), np.array([1.0, 0.5, 2.0]))

    def out(**kw):
        o = eng.ForwardPushOut()
        o.rounds_used, o.converged, o.rem = ints.ctypes.data_as(ip), ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp)
        o.pushes, o.left, o.work = longs.ctypes.data_as(lp), longs.ctypes.data_as(lp), longs.ctypes.data_as(lp)
        o.k, o.min_p = 4, 0.0
        o.topk_ids, o.topk_p, o.topk_counts = ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp), ints.ctypes.data_as(ip)
        o.at_ids, o.n_at, o.at_p, o.at_r = at_ids.ctypes.data_as(ip), 2, dbls.ctypes.data_as(dp), dbls.ctypes.data_as(dp)
        o.dense_p_dev, o.dense_r_dev, o.dense_dtype, o.dense_layout = d_p, d_r, eng.F64, eng.VERTEX_MAJOR
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def refused(csr=good, m=2, eps=1e-6, max_rounds=8, epoch=-1, o=None, **kw):
        o = out(**kw) if o is None else o
        off, ids, w = csr
        rc = L.dppr_forward_push(h, epoch, None if off is None else off.ctypes.data_as(lp), None if ids is None else ids.ctypes.data_as(ip),
                                 None if w is None else w.ctypes.data_as(dp), m, eps, max_rounds, None if o == "null" else C.byref(o))
        clean = (np.all(ints == 77) and np.all(dbls == 7.5) and np.all(longs == 77) and np.all(hip.read(d_p, 8 * 2 * V) == 0xAB)
                 and np.all(hip.read(d_r, 8 * 2 * V) == 0xAB))
        return rc == -1 and bool(clean)

    def csr(off=good[0], ids=good[1], w=good[2]):
        return (None if off is None else np.asarray(off, dtype=np.int64), None if ids is None else np.asarray(ids, dtype=np.int32),
                None if w is None else np.asarray(w, dtype=np.float64))

    bad_id = np.array([1, V], dtype=np.int32)
    too_many = csr([0, 4097, 4098], np.arange(4098) % V, np.ones(4098))
    for kw in (dict(m=0), dict(m=17), dict(m=-1), dict(eps=0.0), dict(eps=-1e-6), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(max_rounds=0), dict(max_rounds=257), dict(o="null"), dict(epoch=1), dict(epoch=7),
               dict(csr=csr(off=None)), dict(csr=csr(ids=None)), dict(csr=csr(w=None)), dict(csr=csr(off=[1, 2, 3])),
               dict(csr=csr(off=[0, 2, 1])), dict(csr=csr(off=[0, 0, 3])), dict(csr=csr(off=[0, 3, 3])), dict(csr=too_many),
               dict(csr=csr(ids=[1, 2, V])), dict(csr=csr(ids=[-1, 2, 5])), dict(csr=csr(ids=[1, 5, 5])),
               dict(csr=csr(w=[1.0, 0.0, 2.0])), dict(csr=csr(w=[1.0, -0.5, 2.0])), dict(csr=csr(w=[1.0, float("nan"), 2.0])),
               dict(csr=csr(w=[float("inf"), 1.0, 2.0])),
               dict(k=0), dict(k=8193), dict(min_p=-1.0), dict(min_p=float("nan")), dict(topk_ids=None), dict(topk_counts=None),
               dict(at_ids=None), dict(at_p=None, at_r=None), dict(n_at=0), dict(n_at=4097), dict(at_ids=bad_id.ctypes.data_as(ip)),
               dict(dense_dtype=2), dict(dense_layout=-1), dict(dense_p_dev=d_p + 4), dict(dense_r_dev=d_r + 8),
               dict(dense_p_dev=ints.ctypes.data)):
        assert refused(**kw), list(kw)
    off, ids, w = good
    args = (off.ctypes.data_as(lp), ids.ctypes.data_as(ip), w.ctypes.data_as(dp), 2, 1e-6, 8)
    assert L.dppr_forward_push(None, -1, *args, C.byref(out())) == -1
    for bad in ((32, 0, 0), (96, 0, 0), (8192, 0, 0), (0, 3, 0), (0, 16, 0), (0, 0, -1), (0, 0, 257)):
        with pytest.raises(eng.DpprError):
            e.debug_forward_push(*bad)
    # the same id in two columns is fine; a call that asks for nothing runs nothing; a part whose pointers are all NULL is not run
    assert L.dppr_forward_push(h, -1, *args[:3], 2, 1e-6, 8, C.byref(eng.ForwardPushOut())) == 0
    only = eng.ForwardPushOut()
    only.rem = dbls.ctypes.data_as(dp)
    assert L.dppr_forward_push(h, -1, *args, C.byref(only)) == 0
    assert np.all(dbls[:2] != 7.5) and np.all(dbls[2:] == 7.5) and np.all(ints == 77) and np.all(longs == 77)
    assert np.all(hip.read(d_p, 8 * 2 * V) == 0xAB) and np.all(hip.read(d_r, 8 * 2 * V) == 0xAB)
    hip.free_all()
    e.close()
