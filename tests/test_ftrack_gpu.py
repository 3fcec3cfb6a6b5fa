"""The forward track (dppr_ftrack_*) on the device against the numpy definition of tests/ftrack_ref.py over the rows the device holds
on every epoch (dppr_read_graph + dppr_debug_id_map) and the records of SlidingStream.batch_arrays(). p and r -- through the top k,
the point reads and the dense copies --, rem, the per-column statistics, `work` and `fix` are compared by bit pattern or as integers;
the tolerances in this file are the derived bounds of the entrywise guarantee and of the bidirectional estimate."""
import ctypes as C

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from dynamicppr_amd.stream import SlidingStream, Workload
from tests import forward_ref as fr
from tests import ftrack_ref as tr
from tests.test_export_gpu import Hip
from tests.test_forward_gpu import bits, rows_of, star
from tests.test_fpush_gpu import WIDTHS, EPSS, as_set
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

WN, C_BATCH, BATCHES, SEED = 4000, 50, 12, 7
META = ("rounds_used", "converged", "pushes", "left")


class Window:
    """An engine over the R-MAT scale-10 stream of tests/test_fpush_gpu.py that slides batch by batch."""

    def __init__(self, directed, n_epochs=2, V=None, e1=None, e2=None, Wn=WN, c=C_BATCH, renumbering=None):
        if V is None:
            V, e1, e2 = datagen.rmat_stream(10, 20000, SEED)
        self.V, self.directed = V, directed
        self.g = SlidingStream(V, e1, e2, directed, Workload(Wn, c, 0, 0))
        self.e = eng.Engine(V, Wn, directed, c, n_epochs=n_epochs)
        if renumbering:
            self.e.set_renumbering(1, **renumbering)
        self.e.load_window(*self.g.serialize_edge_stream())
        self.epoch, self.rows = 0, rows_of(self.e)

    def slide(self):
        """The next epoch: (its batch's records, its rows)."""
        assert not self.g.stream_updates()
        rec = tuple(x.copy() for x in self.g.batch_arrays())
        self.e.set_batch(*rec)
        self.epoch = self.e.slide(*self.g.new_arrays())
        self.rows = rows_of(self.e)
        return rec, self.rows


def standard_sets(w):
    """The columns of the fpush test: hub, sink, a vertex the stream never names, a two-seed set, a 64-seed set with that vertex in
    it, a median-degree vertex; repeated to 16."""
    rows, x2i = w.rows, w.e.id_map()
    hub = int(np.argmax(rows.d))
    e1, e2 = w.g.e1, w.g.e2
    never = np.setdiff1d(np.arange(w.V), np.concatenate([e1[:WN + (BATCHES + 2) * C_BATCH], e2[:WN + (BATCHES + 2) * C_BATCH]]))
    unnamed = int(never[0])
    sink = hub
    if w.directed:
        sink = int(np.nonzero((rows.d == 0) & (np.diff(rows.ptr) > 0))[0][0])
    low = int(np.nonzero((x2i >= 0) & (rows.d == 1))[0][3])
    named = np.nonzero(x2i >= 0)[0]
    rng = np.random.default_rng(11)
    big_ids = np.concatenate([rng.choice(named, 63, replace=False), [unnamed]])
    big = (big_ids[rng.permutation(64)], rng.random(64) + 0.05)
    two = (np.array([hub, low]), np.array([0.25, 3.0]))
    with_out = np.nonzero((x2i >= 0) & (rows.d > 0))[0]
    med = int(with_out[np.argsort(rows.d[with_out], kind="stable")[len(with_out) // 2]])
    return [hub, sink, unnamed, two, big, med, hub, big, sink, two, unnamed, med, hub, two, big, sink], dict(hub=hub, unnamed=unnamed, med=med)


class RefTrack:
    """The reference columns of a track; equal sets share one column."""

    def __init__(self, rows, sets, eps, max_rounds):
        self.uniq, self.order = {}, []
        for s in sets:
            ids, w = as_set(s)
            key = (ids.tobytes(), w.tobytes())
            if key not in self.uniq:
                self.uniq[key] = tr.Column(rows, ids, w, eps, max_rounds)
            self.order.append(key)

    @property
    def cols(self):
        return [self.uniq[k] for k in self.order]

    def update(self, rows, rec, max_rounds):
        for c in self.uniq.values():
            c.update(rows, rec, max_rounds)


def check(what, got, ref, rows, k=40, min_p=0.0, at=None):
    cols = ref.cols
    last = [c.last for c in cols]
    for key in META:
        assert got[key].tolist() == [getattr(l, key) for l in last], (what, key, got[key], [getattr(l, key) for l in last])
    assert np.array_equal(bits(got["rem"]), bits([l.rem for l in last])), (what, got["rem"], [l.rem for l in last])
    assert got["work"].tolist() == tr.work(rows, last).tolist(), (what, got["work"], tr.work(rows, last))
    assert got["fix"].tolist() == last[0].fix, (what, got["fix"], last[0].fix)
    for i, c in enumerate(cols):
        if "topk" in got:
            ids, pk = fr.topk(c.p, k, min_p)
            assert np.array_equal(got["topk"][i][0], ids), (what, i, got["topk"][i][0][:8], ids[:8])
            assert np.array_equal(bits(got["topk"][i][1]), bits(pk)), (what, i)
        if at is not None:
            assert np.array_equal(bits(got["at_p"][i]), bits(c.p[at])), (what, i, "at_p")
            assert np.array_equal(bits(got["at_r"][i]), bits(c.r[at])), (what, i, "at_r")


def check_dense(what, t, ref, hip, V, dtype, layout):
    cols = ref.cols
    m = len(cols)
    size = 4 if dtype == eng.F32 else 8
    ptr = {"p": hip.alloc(size * m * V + 16), "r": hip.alloc(size * m * V + 16)}
    t.read(dense_p_ptr=ptr["p"], dense_r_ptr=ptr["r"], dtype=dtype, layout=layout)
    full = {"p": np.stack([c.p for c in cols]), "r": np.stack([c.r for c in cols])}
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


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_a_fresh_track_is_the_forward_push(directed):
    w = Window(directed)
    e = w.e
    sets, _ = standard_sets(w)
    at = np.arange(w.V, dtype=np.int32)
    for m in WIDTHS:
        for eps, cap in ((1e-6, 64), (1e-8, 5)):
            want = e.forward_push(sets[:m], eps, cap, k=40, at=at)
            t = e.ftrack(sets[:m], eps, cap, k=40, at=at)
            for got in (t.created, t.read(k=40, at=at)):
                for key in META + ("rem", "work", "at_p", "at_r"):
                    assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), (directed, m, eps, key)
                for a, b in zip(got["topk"], want["topk"]):
                    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
                assert got["fix"].tolist() == [0, 0, 0]
            info = t.info()
            assert info["epoch"] == 0 and info["m"] == m and info["eps"] == eps
            for (ids, wt), s in zip(info["sets"], sets[:m]):
                assert np.array_equal(ids, as_set(s)[0]) and np.array_equal(wt, as_set(s)[1])
            t.close()
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_bit_for_bit_after_every_batch(directed):
    w = Window(directed)
    e, V = w.e, w.V
    hip = Hip()
    sets, who = standard_sets(w)
    at = np.arange(0, V, 3, dtype=np.int32)
    tracks = [(e.ftrack(sets, eps, 64), RefTrack(w.rows, sets, eps, 64)) for eps in EPSS]
    for t, ref in tracks:
        check((directed, "create"), t.created, ref, w.rows)
    negative = heads2 = tails2 = same_deg = 0
    for b in range(1, BATCHES + 1):
        d0 = w.rows.d.copy()
        rec, rows = w.slide()
        bt, bh, ins = (np.asarray(x, dtype=np.int64) for x in rec)
        # the preconditions of this test, on the reference
        for u in np.unique(bt):
            tails2 += int(np.sum(bt == u) >= 2)
            same_deg += int(rows.d[u] == d0[u])
        for x in np.unique(bh):
            heads2 += int(len(np.unique(bt[bh == x])) >= 2)
        for t, ref in tracks:
            negative += int(any(np.any(tr.fixup(c.p, c.r, rows.d, bt, bh, ins)[1] < 0) for c in ref.uniq.values()))
            ref.update(rows, rec, 64)
            got = t.update(w.epoch, 64, k=40, at=at)
            check((directed, b, ref.cols[0].eps), got, ref, rows, at=at)
            assert got["fix"][0] == len(bt) == (2 if directed else 4) * C_BATCH
            assert t.info()["epoch"] == w.epoch
            again = t.read(k=40, at=at)   # the counts of the last call, unchanged
            check((directed, b, "read"), again, ref, rows, at=at)
            if b in (1, 7, BATCHES):
                check_dense((directed, b), t, ref, hip, V, eng.F64, eng.VERTEX_MAJOR)
                check_dense((directed, b), t, ref, hip, V, eng.F32, eng.SOURCE_MAJOR)
                check((directed, b, "k = 8192"), t.read(k=8192, min_p=1e-5), ref, rows, k=8192, min_p=1e-5)
    assert negative > 0 and heads2 > 0 and tails2 > 0 and same_deg > 0, (negative, heads2, tails2, same_deg)
    u = tracks[1][1].cols[2]   # the vertex the stream never names: settled exactly, never touched
    assert u.p[who["unnamed"]] == 0.15 and np.count_nonzero(u.p) == 1 and not u.r.any()
    for t, _ in tracks:
        t.close()
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_hub_cut_into_pieces():
    """The star of tests/test_forward_gpu.py (one head of in-degree D) under a stream that deletes and inserts spokes: every
    piece_edges / team / chunk_rounds setting gives the bits of the default one and of numpy."""
    D = 5000
    V, tails, heads, S = star(D)
    rng = np.random.default_rng(D)
    order = rng.permutation(len(tails))
    n, c = len(tails), 40
    extra_t = rng.integers(1, D + 1, 6 * c)      # further spokes tail -> head 0, and S -> tail
    e1 = np.concatenate([tails[order], extra_t]).astype(np.int32)
    e2 = np.concatenate([heads[order], np.where(np.arange(6 * c) % 2 == 0, 0, extra_t)]).astype(np.int32)
    e1[n + 1::2] = S
    sets = [S, (np.array([S, 3]), np.array([2.0, 0.5])), 0]
    at = np.array([0, 1, 2, 3, 4, 5, D, S], dtype=np.int32)
    first = None
    for piece, team, chunk in ((0, 0, 0), (64, 0, 1), (64, 8, 5), (4096, 1, 0), (64, 2, 3)):
        w = Window(1, V=V, e1=e1, e2=e2, Wn=n, c=c)
        w.e.debug_forward_push(piece, team, chunk)
        t = w.e.ftrack(sets, 4e-6, 12, k=8, at=at)
        ref = RefTrack(w.rows, sets, 4e-6, 12) if first is None else None
        blob = [b"".join(np.asarray(t.created[x]).tobytes() for x in ("rem", "at_p", "at_r", "work", "pushes", "left", "rounds_used"))]
        if ref:
            assert np.diff(w.rows.ptr)[0] == D
            check("star create", t.created, ref, w.rows, k=8, at=at)
        for b in range(6):
            rec, rows = w.slide()
            got = t.update(w.epoch, 12, k=8, at=at)
            if ref:
                ref.update(rows, rec, 12)
                check(("star", b), got, ref, rows, k=8, at=at)
            blob.append(b"".join(np.asarray(got[x]).tobytes() for x in ("rem", "at_p", "at_r", "work", "fix", "pushes", "left", "rounds_used")))
        first = blob if first is None else first
        assert blob == first, (piece, team, chunk)
        t.close()
        w.e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_one_round_per_call_reaches_the_bits_of_one_call():
    w = Window(1)
    e = w.e
    sets, _ = standard_sets(w)
    sets = sets[:6]
    at = np.arange(w.V, dtype=np.int32)
    big, step = e.ftrack(sets, 1e-8, 256), e.ftrack(sets, 1e-8, 256)
    ref_big, ref_step = RefTrack(w.rows, sets, 1e-8, 256), RefTrack(w.rows, sets, 1e-8, 256)
    same_history = True
    for b in range(3):
        rec, rows = w.slide()
        ref_big.update(rows, rec, 256)
        check(("big", b), big.update(w.epoch, 256, at=at), ref_big, rows, at=at)
        ref_step.update(rows, rec, 1)   # (b == 2: a fix-up on an unconverged track -- the candidates come from one scan)
        got = step.update(w.epoch, 1, at=at)
        check(("step", b, 0), got, ref_step, rows, at=at)
        assert got["converged"].min() == 0
        calls = 1
        while got["converged"].min() == 0 and not (b == 1 and calls == 3):   # (b == 1: left unconverged)
            ref_step.update(rows, None, 1)
            got = step.update(w.epoch, 1, at=at)
            check(("step", b, calls), got, ref_step, rows, at=at)
            assert got["fix"].tolist() == [0, 0, 0]
            calls += 1
        if b == 1:
            assert got["converged"].min() == 0
            same_history = False
        if same_history:   # as many calls as the rounds of the one call, and its bits
            assert calls == max(c.last.rounds_used for c in ref_big.cols) and calls > 3, calls
            a, z = step.read(at=at), big.read(at=at)
            assert a["at_p"].tobytes() == z["at_p"].tobytes() and a["at_r"].tobytes() == z["at_r"].tobytes()
    assert not same_history
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_track_follows_a_renumbering():
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    w = Window(1, V=V, e1=e1, e2=e2, Wn=W, c=c, renumbering=dict(growth_pct=10, min_parked=16))
    e = w.e
    gid = e.add_source_group([0, 1, 2])   # (a solver that follows the stream, as in tests/test_fpush_gpu.py)
    e.group_init_solve(gid, 1e-9)
    rows = rows_of(e)
    w.rows = rows
    named = np.nonzero((e.id_map() >= 0) & (rows.d > 0))[0]
    # seeds that leave the window for at least 8 batches and are named again: parked by a renumbering in between, then revived
    present = np.zeros((batches + 1, V), dtype=bool)
    for k in range(batches + 1):
        present[k, e1[k * c:k * c + W]] = present[k, e2[k * c:k * c + W]] = True
    back = []
    for v in np.nonzero(present[0] & (rows.d > 0))[0]:
        gone = np.nonzero(~present[:, v])[0]
        again = np.nonzero(present[gone[0]:, v])[0] if len(gone) else []
        if len(again) and again[0] >= 8:
            back.append(int(v))
    assert len(back) >= 6
    sets = [int(named[0]), (named[[3, 50, 200]], np.array([1.0, 0.7, 2.0])), int(np.argmax(rows.d)), int(named[-1]),
            (np.array(back[:6]), np.array([1.0, 0.5, 2.0, 1.5, 0.75, 1.25]))]
    at = np.arange(V, dtype=np.int32)
    t, ref = e.ftrack(sets, 1e-6, 64, at=at), RefTrack(rows, sets, 1e-6, 64)
    check("churn create", t.created, ref, rows, at=at)
    r0 = e.id_space()["renumberings"]
    parked_seed = revived = 0
    seeds = np.unique(np.concatenate([as_set(s)[0] for s in sets]))
    was_parked = np.zeros(V, dtype=bool)
    for b in range(batches):
        rec, rows = w.slide()
        e.group_update(gid, 1e-9)
        ref.update(rows, rec, 64)
        got = t.update(w.epoch, 64, k=20, at=at)
        if b % 6 == 0 or b > batches - 4:
            check(("churn", b), got, ref, rows, k=20, at=at)
        else:
            assert np.array_equal(bits(got["at_p"]), bits(np.stack([c.p for c in ref.cols]))), b
            assert np.array_equal(bits(got["at_r"]), bits(np.stack([c.r for c in ref.cols]))), b
        sp, x2i = e.id_space(), e.id_map()
        now_parked = x2i >= V - sp["parked"]
        parked_seed += int(now_parked[seeds].any())
        revived += int(np.any(was_parked[seeds] & ~now_parked[seeds]))
        if now_parked[seeds].any():   # a parked seed keeps its values
            q = seeds[now_parked[seeds]][0]
            assert any(c.p[q] != 0.0 for c in ref.cols)
        was_parked = now_parked
    sp = e.id_space()
    assert sp["renumberings"] > r0 and sp["parked"] > 0, sp
    print("churn: renumberings", sp["renumberings"] - r0, "batches with a parked seed", parked_seed, "revivals of a seed", revived)
    assert parked_seed > 0 and revived > 0
    t.close()
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_both_directions_hold_together():
    """After each batch |p_track - p_fresh| <= rem_track + rem_fresh entrywise (both are within their rem of pihat_h; the signed
    track on either side, the fresh push below). Against a source group solved at EPS: pihat_h(s) = p[s] + sum_u r[u] pihat_u(s)
    exactly, the group holds |p_i[u] - pihat_u(s_i)| <= EPS, f_256 of dppr_forward is below pihat by at most rem_256, and 1e-12
    covers the rounding of the sums: |p[s_i] + group_dot(r)[i] - f_256[s_i]| <= rem * EPS + rem_256 + 1e-12. Derived, not tuned."""
    EPS = 1e-9
    w = Window(1)
    e, V = w.e, w.V
    hip = Hip()
    srcs = [int(x) for x in datagen.top_sources(V, w.g.e1, w.g.e2, WN, 1, 10)]
    gid = e.add_source_group(srcs)
    e.group_init_solve(gid, EPS)
    named = np.nonzero((e.id_map() >= 0) & (w.rows.d > 0))[0]
    q = [int(x) for x in np.random.default_rng(17).choice(named, 8, replace=False)]
    at = np.arange(V, dtype=np.int32)
    d_r = hip.alloc(8 * len(q) * V)
    t = e.ftrack(q, 1e-6, 64)
    for b in range(4):
        w.slide()
        e.group_update(gid, EPS)
        got = t.update(w.epoch, 64, at=at, dense_r_ptr=d_r, dtype=eng.F64, layout=eng.SOURCE_MAJOR)
        fresh = e.forward_push(q, 1e-6, 64, at=at)
        gap = np.abs(got["at_p"] - fresh["at_p"])
        bound = (got["rem"] + fresh["rem"])[:, None]
        print("ftrack vs fresh", b, "largest gap", gap.max(), "smallest bound", bound.min())
        assert np.all(gap <= bound) and np.all(got["converged"] == 1)
        f = e.forward(np.array(q, dtype=np.int32), 256, 0.0, at=np.array(srcs, dtype=np.int32))
        dot = e.group_dot_dense_dev(gid, d_r, len(q))
        est = got["at_p"][:, srcs] + dot
        gap2 = np.abs(est - f["at"])
        bound2 = (got["rem"] * EPS + f["rem"] + 1e-12)[:, None]
        print("ftrack bidirectional", b, "largest gap", gap2.max(), "smallest bound", bound2.min())
        assert np.all(gap2 <= bound2)
    hip.free_all()
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_column_alone_and_among_sixteen_and_beside_the_solver():
    w = Window(1)
    e = w.e
    sets, _ = standard_sets(w)
    at = np.arange(w.V, dtype=np.int32)
    gid = e.add_source_group([int(np.argmax(w.rows.d)), 1, 2])
    e.group_init_solve(gid, 1e-7)
    together = e.ftrack(sets, 1e-6, 10)
    alone = {i: e.ftrack(sets[i:i + 1], 1e-6, 10) for i in (0, 4, 15)}
    for b in range(3):
        w.slide()
        if b != 1:
            e.group_update(gid, 1e-7)   # (b == 1: the solver skips the epoch's update for now; nothing of a track depends on it)
        before = [x.tobytes() for x in e.group_read(gid, 0)]
        got = together.update(w.epoch, 10, at=at)
        assert [x.tobytes() for x in e.group_read(gid, 0)] == before   # no state is changed
        for i, t in alone.items():
            one = t.update(w.epoch, 10, at=at)
            for key in META + ("rem",):
                assert np.asarray(one[key])[0].tobytes() == np.asarray(got[key])[i].tobytes(), (b, i, key)
            assert one["at_p"][0].tobytes() == got["at_p"][i].tobytes() and one["at_r"][0].tobytes() == got["at_r"][i].tobytes(), (b, i)
            assert one["fix"].tolist() == got["fix"].tolist()
        if b == 1:
            e.group_update(gid, 1e-7)
    e.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_an_update_gathers_fewer_rows_than_a_fresh_push():
    w = Window(1)
    e = w.e
    sets, who = standard_sets(w)
    med = [who["med"]]
    t, ref = e.ftrack(med, 1e-6, 64), RefTrack(w.rows, med, 1e-6, 64)
    fewer = 0
    for b in range(BATCHES):
        rec, rows = w.slide()
        ref.update(rows, rec, 64)
        got = t.update(w.epoch, 64)
        want = tr.work(rows, [c.last for c in ref.cols])
        assert got["work"].tolist() == want.tolist()
        fresh_ref = tr.work(rows, [tr.Column(rows, *as_set(med[0]), 1e-6, 64).last])
        fresh = e.forward_push(med, 1e-6, 64)["work"]
        assert fresh.tolist() == fresh_ref.tolist()
        if want[1] < fresh_ref[1]:   # where the reference shows it, the device shows it
            assert got["work"][1] < fresh[1]
            fewer += 1
        print("locality", b, "update", got["work"].tolist(), "fresh", fresh.tolist())
    assert fewer >= BATCHES // 2, fewer
    e.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_track_and_the_outputs_untouched():
    w = Window(1, n_epochs=2)
    e, V = w.e, w.V
    hip = Hip()
    L, h = e._L, e._h
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    ints, dbls, longs = np.full(64, 77, dtype=np.int32), np.full(64, 7.5), np.full(64, 77, dtype=np.int64)
    d_p, d_r = hip.alloc(8 * 2 * V), hip.alloc(8 * 2 * V)
    at_ids = np.array([1, 2], dtype=np.int32)
    good = (np.array([0, 1, 3], dtype=np.int64), np.array([1, 2, 5], dtype=np.int32), np.array([1.0, 0.5, 2.0]))
    handle = C.c_int32(-5)

    def out(**kw):
        o = eng.FtrackOut()
        o.rounds_used, o.converged, o.rem = ints.ctypes.data_as(ip), ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp)
        o.pushes, o.left, o.work, o.fix = longs.ctypes.data_as(lp), longs.ctypes.data_as(lp), longs.ctypes.data_as(lp), longs.ctypes.data_as(lp)
        o.k, o.min_p = 4, 0.0
        o.topk_ids, o.topk_p, o.topk_counts = ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp), ints.ctypes.data_as(ip)
        o.at_ids, o.n_at, o.at_p, o.at_r = at_ids.ctypes.data_as(ip), 2, dbls.ctypes.data_as(dp), dbls.ctypes.data_as(dp)
        o.dense_p_dev, o.dense_r_dev, o.dense_dtype, o.dense_layout = d_p, d_r, eng.F64, eng.VERTEX_MAJOR
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def clean():
        return bool(np.all(ints == 77) and np.all(dbls == 7.5) and np.all(longs == 77) and np.all(hip.read(d_p, 8 * 2 * V) == 0xAB)
                    and np.all(hip.read(d_r, 8 * 2 * V) == 0xAB))

    def create_refused(csr=good, m=2, eps=1e-6, max_rounds=8, epoch=-1, track="ptr", **kw):
        off, ids, wt = csr
        rc = L.dppr_ftrack_create(h, epoch, None if off is None else off.ctypes.data_as(lp), None if ids is None else ids.ctypes.data_as(ip),
                                  None if wt is None else wt.ctypes.data_as(dp), m, eps, max_rounds, C.byref(out(**kw)),
                                  C.byref(handle) if track == "ptr" else None)
        return rc == -1 and clean() and handle.value == -5

    def csr(off=good[0], ids=good[1], wt=good[2]):
        return (None if off is None else np.asarray(off, dtype=np.int64), None if ids is None else np.asarray(ids, dtype=np.int32),
                None if wt is None else np.asarray(wt, dtype=np.float64))

    bad_id = np.array([1, V], dtype=np.int32)
    too_many = csr([0, 4097, 4098], np.arange(4098) % V, np.ones(4098))
    bad_outs = (dict(k=0), dict(k=8193), dict(min_p=-1.0), dict(min_p=float("nan")), dict(topk_ids=None), dict(topk_counts=None),
                dict(at_ids=None), dict(at_p=None, at_r=None), dict(n_at=0), dict(n_at=4097), dict(at_ids=bad_id.ctypes.data_as(ip)),
                dict(dense_dtype=2), dict(dense_layout=-1), dict(dense_p_dev=d_p + 4), dict(dense_r_dev=d_r + 8), dict(dense_p_dev=ints.ctypes.data))
    for kw in (dict(m=0), dict(m=17), dict(m=-1), dict(eps=0.0), dict(eps=-1e-6), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(max_rounds=0), dict(max_rounds=257), dict(track=None), dict(epoch=1), dict(epoch=7),
               dict(csr=csr(off=None)), dict(csr=csr(ids=None)), dict(csr=csr(wt=None)), dict(csr=csr(off=[1, 2, 3])),
               dict(csr=csr(off=[0, 2, 1])), dict(csr=csr(off=[0, 0, 3])), dict(csr=csr(off=[0, 3, 3])), dict(csr=too_many),
               dict(csr=csr(ids=[1, 2, V])), dict(csr=csr(ids=[-1, 2, 5])), dict(csr=csr(ids=[1, 5, 5])),
               dict(csr=csr(wt=[1.0, 0.0, 2.0])), dict(csr=csr(wt=[1.0, -0.5, 2.0])), dict(csr=csr(wt=[1.0, float("nan"), 2.0])),
               dict(csr=csr(wt=[float("inf"), 1.0, 2.0]))) + bad_outs:
        assert create_refused(**kw), list(kw)
    sets = [1, (np.array([2, 5]), np.array([0.5, 2.0]))]
    at = np.arange(V, dtype=np.int32)
    t = e.ftrack(sets, 1e-6, 8)
    state = t.read(at=at)

    def unchanged():
        now = t.read(at=at)
        return clean() and t.info()["epoch"] == 0 and all(np.asarray(now[x]).tobytes() == np.asarray(state[x]).tobytes() for x in state)

    def update_refused(track=None, epoch=-1, max_rounds=8, **kw):
        rc = L.dppr_ftrack_update(h, t.handle if track is None else track, epoch, max_rounds, C.byref(out(**kw)))
        return rc == -1 and unchanged()

    for kw in bad_outs:
        assert update_refused(**kw), list(kw)
        assert L.dppr_ftrack_read(h, t.handle, C.byref(out(**kw))) == -1 and unchanged(), list(kw)
    assert update_refused(max_rounds=0) and update_refused(max_rounds=257) and update_refused(track=-1) and update_refused(track=16)
    assert update_refused(track=t.handle + 1) and update_refused(epoch=1)   # no such track; an epoch that was never built
    assert L.dppr_ftrack_read(h, t.handle, None) == -1 and L.dppr_ftrack_read(h, 9, C.byref(out())) == -1 and unchanged()
    w.slide()
    w.slide()                                                   # epochs 1 and 2 are resident (n_epochs = 2), 0 is not
    assert update_refused(epoch=2), "a skipped epoch"
    assert update_refused(epoch=0), "the own epoch, no longer resident"
    t.update(1, 8)
    t.update(2, 8, k=4, at=at)
    state = t.read(at=at)

    def unchanged():   # noqa: F811  (the track stands on epoch 2 now)
        now = t.read(at=at)
        return clean() and t.info()["epoch"] == 2 and all(np.asarray(now[x]).tobytes() == np.asarray(state[x]).tobytes() for x in state)

    assert update_refused(epoch=1), "a replayed older epoch"
    assert update_refused(epoch=4), "an epoch that does not exist yet"
    # a 17th track
    others = [e.ftrack([3], 1e-4, 4) for _ in range(eng.FTRACK_MAX - 1)]
    assert sorted([t.handle] + [o.handle for o in others]) == list(range(16))
    assert create_refused() and unchanged()
    for o in others:
        o.close()
    gone = t.handle
    t.close()
    assert L.dppr_ftrack_update(h, gone, -1, 8, C.byref(out())) == -1 and L.dppr_ftrack_read(h, gone, C.byref(out())) == -1 and clean()
    assert L.dppr_ftrack_destroy(h, gone) == -1 and L.dppr_ftrack_info(h, gone, None, None, None, None, None, None, 0) == -1
    # a track that comes and goes leaves the bytes where they were (the work space is the engine's: the tracks above have sized it)
    w.slide()
    w.slide()
    base = eng.live_bytes()
    t2 = e.ftrack(sets, 1e-6, 8, k=4, at=at, epoch=w.epoch - 1)
    assert t2.handle == 0 and eng.live_bytes()[0] >= base[0] + 2 * 8 * 2 * V   # (a freed handle is handed out again)
    t2.update(w.epoch, 8, k=4, at=at)
    t2.close()
    assert eng.live_bytes() == base
    hip.free_all()
    e.close()
