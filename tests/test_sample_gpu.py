"""Vertices drawn in proportion to a lane's score (dppr_sample / dppr_group_sample) against the numpy restatement of
tests/sample_ref.py over what the engine reports through its other calls: the dense columns from group_read / read, the out-CSR of
the epoch by external id from read_out_graph, with the scores of tests/rank_ref.py. Every step of the definition is one IEEE
operation, so every comparison is array_equal: on the ids, and on the bit patterns of the weights and the totals."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import rank_ref, sample_ref
from tests.sample_ref import bits
from tests.test_dot_gpu import put
from tests.test_export_gpu import Hip
from tests.test_rank_gpu import IN, OUT, S as SEEDS, cols_of, graph_of
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

EPS = 1e-9
WIDTHS = (1, 5, 8, 10, 16)
V_SMALL, W_SMALL, C_SMALL = 5001, 6000, 60
FIRSTS = (0, 2 ** 32 - 3)
MIN_SCORES = (0.0, 1e-4)
SEED = 0x5EED0123456789AB


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


class Window:
    """An R-MAT scale 12 stream (ids below 4096) on an engine of V = 5001: 905 ids never get an internal id, the last tile holds
    905 ids, its last subtile is partial, P = 8192. One group per width and one slot; renumbering on."""

    def __init__(self):
        V0, e1, e2 = datagen.rmat_stream(12, W_SMALL + 10 * C_SMALL, 7)
        assert V0 == 4096
        self.V = V_SMALL
        self.srcs = [int(x) for x in datagen.top_sources(V0, e1, e2, W_SMALL, 1, 16)]
        self.g = orc.Graph(self.V, e1, e2, 1, W_SMALL, C_SMALL)
        self.e = eng.Engine(self.V, W_SMALL, 1, C_SMALL)
        self.e.set_renumbering(1, growth_pct=10, min_parked=16)
        self.e.load_window(*self.g.window_edges())
        self.groups = {n: self.e.add_source_group(self.srcs[:n]) for n in WIDTHS}
        self.slot = self.e.add_source(self.srcs[0])
        for gid in self.groups.values():
            self.e.group_init_solve(gid, EPS)
        self.e.init_solve(self.slot, EPS)
        self.updates = 0

    def update(self, batches):
        for _ in range(batches):
            assert not self.g.stream_updates()
            self.g.inc_construct(1)
            self.e.set_batch(*self.g.batch())
            self.e.slide(*self.g.new_stream())
            for gid in self.groups.values():
                self.e.group_update(gid, EPS)
            self.e.update(self.slot, EPS)
        self.updates += batches


@pytest.fixture(scope="module")
def win():
    """The first test looks at the init state and then takes two updates; every later test sees the state after them (the tests
    of this module run in file order)."""
    w = Window()
    yield w
    w.e.close()


def updated(w):
    if w.updates == 0:
        w.update(2)
    return w


def same(got, want, what):
    ids, wt, total, support, status = got
    rid, rw, rtotal, rsupport, rstatus = want
    assert ids.dtype == np.int32 and ids.shape == rid.shape, what
    assert np.array_equal(bits(total), bits(rtotal)), (what, "total", total, rtotal)
    assert np.array_equal(support, rsupport) and np.array_equal(status, rstatus), (what, support, rsupport, status, rstatus)
    assert np.array_equal(ids, rid), (what, "ids", np.argwhere(ids != rid)[:4])
    if wt is not None:
        assert wt.dtype == np.float64 and np.array_equal(bits(wt), bits(rw)), (what, "w")


def check(e, gid, spec, want, what, Ss=(1000, 1), firsts=FIRSTS, min_scores=MIN_SCORES, seed=SEED):
    """group_sample against the reference over the scores `want` (one [V] array per lane); returns the last result."""
    sc = np.stack(want, axis=1)
    got = None
    for S in Ss:
        for first in firsts:
            for ms in min_scores:
                got = e.group_sample(gid, S, spec, ms, seed, first)
                same(got, sample_ref.group_sample(sc, S, ms, seed, first), (what, S, first, ms))
    return got


def anchor_a(e, gid, spec, ids, w, ms, what):
    """Every drawn id has group_rank_score_at in its lane equal to out_w bit for bit, and > min_score."""
    for i in range(ids.shape[0]):
        drawn = ids[i][ids[i] >= 0]
        if len(drawn) == 0:
            continue
        back = e.group_rank_score_at(gid, drawn, spec)[:, i]
        assert np.array_equal(bits(back), bits(w[i][ids[i] >= 0])) and np.all(back > ms), (what, i)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_width_after_init_and_after_two_updates(win):
    w = win
    e = w.e
    for state in ("init", "two updates"):
        if state != "init":
            updated(w)
        id_map = e.id_map()
        assert np.count_nonzero(id_map < 0) >= V_SMALL - 4096        # ids without an internal id
        for n, gid in w.groups.items():
            cols = cols_of(e, gid, n)
            for ms in MIN_SCORES:
                ids, wt, total, support, status = e.group_sample(gid, 1000, None, ms, SEED, 0)
                assert np.all(status == eng.SAMPLE_OK) and np.all(ids >= 0) and np.all(ids < 4096) and np.all(wt > ms)
                anchor_a(e, gid, None, ids, wt, ms, (state, n, ms))
            got = check(e, gid, None, cols, (state, n))
            assert got[0].shape == (n, 1)
            # (b) the draws of (first, a + b) are those of (first, a) followed by those of (first + a, b), also across the 32-bit word
            for first in FIRSTS:
                whole = e.group_sample(gid, 1000, None, 0.0, SEED, first)
                head, tail = e.group_sample(gid, 400, None, 0.0, SEED, first), e.group_sample(gid, 600, None, 0.0, SEED, first + 400)
                assert np.array_equal(whole[0], np.concatenate([head[0], tail[0]], axis=1)), (state, n, first)
                assert np.array_equal(bits(whole[1]), bits(np.concatenate([head[1], tail[1]], axis=1)))
            # a lane's draws do not depend on the seeds of the other lanes' draws, but they do on the seed
            assert not np.array_equal(e.group_sample(gid, 1000, None, 0.0, SEED + 1, 0)[0], e.group_sample(gid, 1000, None, 0.0, SEED, 0)[0])
        # the slot is lane 0 of a group of one over the same source
        p = e.read(w.slot)[0]
        for S in (1000, 1):
            for first in FIRSTS:
                for ms in MIN_SCORES:
                    ids, wt, total, support, status = e.sample(w.slot, S, None, ms, SEED, first)
                    rid, rw, rt, rs, rst = sample_ref.group_sample(p[:, None], S, ms, SEED, first)
                    assert np.array_equal(ids, rid[0]) and np.array_equal(bits(wt), bits(rw[0])), (state, "slot", S, first, ms)
                    assert bits(np.array([total]))[0] == bits(rt)[0] and support == rs[0] and status == rst[0]
    assert w.updates == 2


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_specs_of_the_ranked_family(win, hip):
    w = updated(win)
    e, V = w.e, w.V
    tails, heads, deg = graph_of(e)
    rng = np.random.default_rng(12)
    for n in WIDTHS:
        gid = w.groups[n]
        cols = cols_of(e, gid, n)
        seeds = [[x] for x in w.srcs[:n]]
        # the degree factor with the seeds and their in-neighbours left out, per lane
        ex = rank_ref.excluded(V, tails, heads, seeds, SEEDS | IN)
        spec = eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=SEEDS | IN)
        want = rank_ref.scores(cols, rank_ref.DEG, outdeg=deg, excl=ex)
        ids, wt, _, _, _ = check(e, gid, spec, want, (n, "deg + seeds, in"), Ss=(1000,))
        for i in range(n):
            assert not ex[i][ids[i]].any()
        anchor_a(e, gid, spec, ids, wt, 1e-4, (n, "deg"))
        # a float32 factor by external id with zeros and one negative entry
        g = (rng.random(V) * 4.0 + 0.01).astype(np.float32)
        g[rng.random(V) < 0.2] = 0.0
        top = np.argsort(-cols[0])[:4]
        g[top[0]] = -2.0
        g[top[1]] = 3.0
        spec = eng.Engine.rank_spec(eng.FACTOR_DEV, put(hip, g), eng.F32)
        want = rank_ref.scores(cols, rank_ref.DEV, g=g)
        assert (want[0] < 0).any()
        ids, wt, _, _, _ = check(e, gid, spec, want, (n, "dev f32"), Ss=(1000,), firsts=(0,))
        assert np.all(g[ids] > 0) and top[0] not in ids[0]
        # (c) a mask that leaves one vertex: every draw of a lane that holds it is that vertex
        only = int(top[1])
        allow = np.zeros(V, dtype=np.uint8)
        allow[only] = 1
        spec = eng.Engine.rank_spec(mask=eng.MASK_ALLOW, mask_dev=put(hip, allow))
        want = rank_ref.scores(cols, allow=allow)
        ids, wt, total, support, status = check(e, gid, spec, want, (n, "one vertex"), Ss=(1000,), firsts=(0,), min_scores=(0.0,))
        assert status[0] == eng.SAMPLE_OK and support[0] == 1 and np.all(ids[0] == only) and np.all(bits(wt[0]) == bits(cols[0][only:only + 1])[0])
        # ... and one that leaves none: EMPTY, every id -1, the total +0.0
        spec = eng.Engine.rank_spec(mask=eng.MASK_ALLOW, mask_dev=put(hip, np.zeros(V, dtype=np.uint8)))
        ids, wt, total, support, status = check(e, gid, spec, [np.zeros(V)] * n, (n, "nothing"), Ss=(1000,), firsts=(0,), min_scores=(0.0,))
        assert np.all(status == eng.SAMPLE_EMPTY) and np.all(ids == -1) and np.all(bits(total) == 0) and np.all(bits(wt) == 0) and np.all(support == 0)
        # a factor with one +inf: NONFINITE in the lanes where that vertex has p > 0
        g = np.ones(V)
        g[only] = np.inf
        spec = eng.Engine.rank_spec(eng.FACTOR_DEV, put(hip, g), eng.F64)
        want = rank_ref.scores(cols, rank_ref.DEV, g=g)
        ids, wt, total, support, status = check(e, gid, spec, want, (n, "inf"), Ss=(1000,), firsts=(0,), min_scores=(0.0,))
        hit = np.array([c[only] > 0 for c in cols])
        assert hit[0] and np.array_equal(status == eng.SAMPLE_NONFINITE, hit) and np.all(ids[hit] == -1) and np.all(np.isinf(total[hit]))
        assert np.all(ids[~hit] >= 0)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_forms_repeats_and_optional_outputs(win):
    w = updated(win)
    e, V = w.e, w.V
    tails, heads, deg = graph_of(e)
    for n in (1, 10, 16):
        gid = w.groups[n]
        cols = cols_of(e, gid, n)
        spec = eng.Engine.rank_spec(eng.FACTOR_INV_DEG, exclude=SEEDS | OUT)
        want = rank_ref.scores(cols, rank_ref.INV_DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, [[x] for x in w.srcs[:n]], SEEDS | OUT))
        runs = []
        for form in (eng.SAMPLE_WAVE, eng.SAMPLE_PER_THREAD, eng.SAMPLE_WAVE):
            e.debug_sample_form(form)
            runs.append(check(e, gid, spec, want, (n, "form", form), Ss=(1000,)))
            runs.append(check(e, gid, spec, want, (n, "form", form, "S = 1"), Ss=(1,), firsts=(5,)))
        e.debug_sample_form(eng.SAMPLE_WAVE)
        for other in runs[2::2]:
            assert all(np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b) for a, b in zip(other, runs[0]))
        # two identical calls give identical bits
        a, b = e.group_sample(gid, 1000, spec, 0.0, 3, 7), e.group_sample(gid, 1000, spec, 0.0, 3, 7)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2]))
        # (d) S == 0: totals, supports and statuses alone
        ids, wt, total, support, status = e.group_sample(gid, 0, spec, 0.0, 3, 7)
        assert ids.shape == (n, 0) and np.array_equal(bits(total), bits(a[2])) and np.array_equal(support, a[3]) and np.array_equal(status, a[4])
        assert np.array_equal(support, [np.count_nonzero(s > 0) for s in want])
        guard_t, guard_s = np.full(n, 7.5), np.full(n, 77, dtype=np.int32)
        assert e._L.dppr_group_sample(e._h, gid, -1, C.byref(spec), 0.0, 3, 7, 0, eng.DEST_HOST, None, None, guard_t.ctypes.data_as(C.POINTER(C.c_double)),
                                      None, guard_s.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        assert np.array_equal(bits(guard_t), bits(a[2])) and np.array_equal(guard_s, a[4])
        # out_w == NULL
        ids, wt, total, support, status = e.group_sample(gid, 1000, spec, 0.0, 3, 7, with_w=False)
        assert wt is None and np.array_equal(ids, a[0])
    for bad in (-1, 2):
        with pytest.raises(eng.DpprError):
            e.debug_sample_form(bad)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_parked_and_unnamed_vertices(hip):
    """The churn stream of tests/test_rank_gpu.py, renumbering on: parked vertices keep a positive weight and are drawn by their
    external id, ids without an internal id never are."""
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    gid = e.add_source_group([0, 1, 2])
    e.group_init_solve(gid, EPS)
    for _ in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.group_update(gid, EPS)
    sp = e.id_space()
    assert sp["parked"] > 0 and sp["renumberings"] > 0, sp
    id_map = e.id_map()
    unnamed = np.nonzero(id_map < 0)[0]
    parked = np.nonzero(id_map >= V - sp["parked"])[0]
    cols = cols_of(e, gid, 3)
    assert len(unnamed) > 0 and any(np.any(col[parked] > 0) for col in cols)
    tails, heads, deg = graph_of(e)
    for what, spec, kw in (("plain", None, {}),
                           ("deg + all", eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=SEEDS | IN | OUT),
                            dict(factor=rank_ref.DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, [[0], [1], [2]], SEEDS | IN | OUT)))):
        want = rank_ref.scores(cols, **kw)
        ids = check(e, gid, spec, want, ("churn", what), Ss=(4000,), firsts=(0,), min_scores=(0.0,))[0]
        assert not np.isin(ids, unnamed).any()
    # the parked vertices alone (a mask allows nothing else): they are drawn, by their external ids
    allow = np.zeros(V, dtype=np.uint8)
    allow[parked] = 1
    want = rank_ref.scores(cols, allow=allow)
    ids, _, _, support, status = check(e, gid, eng.Engine.rank_spec(mask=eng.MASK_ALLOW, mask_dev=put(hip, allow)), want, ("churn", "parked alone"),
                                       Ss=(500,), firsts=(0,), min_scores=(0.0,))
    assert (status == eng.SAMPLE_OK).any()
    for i in range(3):
        assert support[i] == np.count_nonzero(cols[i][parked] > 0) and (status[i] != eng.SAMPLE_OK or np.isin(ids[i], parked).all())
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_tree_of_17_levels_and_35_tiles():
    """R-MAT scale 16 on V = 70 001: P = 2^17, 35 tiles, so the levels above a tile hold 18, 9, 5, 3, 2 and 1 nodes: odd tails."""
    V, W = 70001, 70000
    V0, e1, e2 = datagen.rmat_stream(16, W, 3)
    assert V0 == 65536
    e = eng.Engine(V, W, 1, 700)
    e.load_window(e1[:W], e2[:W])
    srcs = [int(x) for x in datagen.top_sources(V0, e1, e2, W, 1, 10)]
    gid = e.add_source_group(srcs)
    e.group_init_solve(gid, EPS)
    cols = cols_of(e, gid, 10)
    tails, heads, deg = graph_of(e)
    assert max(int(np.nonzero(c)[0].max()) for c in cols) > 65536 - 2048        # the tile before the empty ones is in use
    spec = eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=SEEDS | IN)
    want = rank_ref.scores(cols, rank_ref.DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, [[x] for x in srcs], SEEDS | IN))
    assert len(sample_ref.tree(sample_ref.weights(want[0]))) == 18               # levels 0 .. 17
    for form in (eng.SAMPLE_WAVE, eng.SAMPLE_PER_THREAD):
        e.debug_sample_form(form)
        ids, wt, _, _, _ = check(e, gid, spec, want, ("2^16", form), Ss=(4096,), firsts=(0,), min_scores=(0.0,))
    anchor_a(e, gid, spec, ids, wt, 0.0, "2^16")
    # the last id of all: a weight there makes the last, partial tile and the odd tails of the upper levels carry a draw
    g = np.zeros(V)
    g[V - 1] = 1.0
    g[srcs[0]] = 1.0
    e.debug_sample_form(eng.SAMPLE_WAVE)
    h = Hip()
    try:
        spec = eng.Engine.rank_spec(eng.FACTOR_DEV, put(h, g), eng.F64)
        check(e, gid, spec, rank_ref.scores(cols, rank_ref.DEV, g=g), "last id", Ss=(64,), firsts=(0,), min_scores=(0.0,))
    finally:
        h.free_all()
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_on_a_live_engine(win, hip):
    w = updated(win)
    e, V = w.e, w.V
    L, h = e._L, e._h
    gid, slot = w.groups[10], w.slot
    n, S = 10, 8
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ids, wt = np.full(n * S, 77, dtype=np.int32), np.full(n * S, 7.5)
    total, support, status = np.full(n, 7.5), np.full(n, 77, dtype=np.int32), np.full(n, 77, dtype=np.int32)
    d_ids, d_w = hip.alloc(4 * n * S), hip.alloc(8 * n * S)

    def untouched():
        return bool(np.all(ids == 77) and np.all(wt == 7.5) and np.all(total == 7.5) and np.all(support == 77) and np.all(status == 77))

    def refused(spec=None, epoch=-1, ms=0.0, first=0, S_=S, dest=eng.DEST_HOST, out=ids.ctypes.data, out_w=wt.ctypes.data, tot=total.ctypes.data_as(dp),
                stat=status.ctypes.data_as(ip), group=gid, slot_=slot):
        sp = C.byref(spec) if spec is not None else None
        sup = support.ctypes.data_as(ip)
        rcs = (L.dppr_group_sample(h, group, epoch, sp, ms, 1, first, S_, dest, out, out_w, tot, sup, stat),
               L.dppr_sample(h, slot_, epoch, sp, ms, 1, first, S_, dest, out, out_w, tot, sup, stat))
        return rcs == (-1, -1) and untouched()

    top = 2 ** 64 - 1
    for kw in (dict(ms=-1e-300), dict(ms=float("nan")), dict(S_=-1), dict(S_=eng.SAMPLE_MAX + 1), dict(first=top - S + 1), dict(first=top),
               dict(dest=2), dict(dest=-1), dict(out=None), dict(tot=None), dict(stat=None), dict(group=99, slot_=99), dict(group=-1, slot_=-1),
               dict(dest=eng.DEST_DEVICE, out=ids.ctypes.data, out_w=None),            # host memory named as a device destination
               dict(dest=eng.DEST_DEVICE, out=d_ids + 2, out_w=None),                   # misaligned
               dict(dest=eng.DEST_DEVICE, out=d_ids, out_w=wt.ctypes.data),             # w on the host
               dict(dest=eng.DEST_DEVICE, out=d_ids, out_w=d_w + 4)):
        assert refused(**kw), list(kw)
    # (n * S > DPPR_SAMPLE_MAX_TOTAL cannot be reached on an engine: 16 lanes at S = DPPR_SAMPLE_MAX are exactly 2^24 draws; the rule is
    # held at its limit by tests/native/sample_plan_test.cpp)
    assert 16 * eng.SAMPLE_MAX == eng.SAMPLE_MAX_TOTAL
    # a device destination that is too small for n * S
    small = hip.alloc(4 * n * S - 4)
    assert L.dppr_group_sample(h, gid, -1, None, 0.0, 1, 0, S, eng.DEST_DEVICE, small, None, total.ctypes.data_as(dp), None, status.ctypes.data_as(ip)) == -1
    assert untouched()
    # every spec rejection of dppr_topk_ranked
    spec = eng.Engine.rank_spec
    g64 = np.ones(V)
    d_g = put(hip, g64)
    d_mask = put(hip, np.zeros(V, dtype=np.uint8))
    for sp in (spec(eng.FACTOR_DEV, g64.ctypes.data), spec(eng.FACTOR_DEV, 0), spec(eng.FACTOR_DEV, put(hip, np.ones(V - 1))),
               spec(eng.FACTOR_DEV, d_g + 4), spec(eng.FACTOR_DEV, d_g, 2), spec(mask=eng.MASK_ALLOW, mask_dev=g64.ctypes.data),
               spec(mask=eng.MASK_DENY, mask_dev=d_mask + 1), spec(4), spec(-1), spec(mask=3), spec(exclude=8)):
        assert refused(sp), (sp.factor, sp.factor_dtype, sp.mask, sp.exclude)
    # ... and its epoch rejection where the spec needs one
    for sp in (spec(eng.FACTOR_DEG), spec(eng.FACTOR_INV_DEG), spec(exclude=IN), spec(exclude=OUT)):
        assert refused(sp, 10 ** 6) and b"not resident" in L.dppr_last_error(h)
    # the limits themselves are accepted, and a valid call writes exactly the documented shape
    assert L.dppr_group_sample(h, gid, -1, None, 0.0, 1, top - S, S - 1, eng.DEST_HOST, ids.ctypes.data, wt.ctypes.data, total.ctypes.data_as(dp),
                               support.ctypes.data_as(ip), status.ctypes.data_as(ip)) == 0
    assert np.all(ids[:n * (S - 1)] >= 0) and np.all(ids[n * (S - 1):] == 77) and np.all(wt[n * (S - 1):] == 7.5) and np.all(status == 0)
    got = e.group_sample(gid, S - 1, None, 0.0, 1, top - S)
    assert np.array_equal(ids[:n * (S - 1)].reshape(n, S - 1), got[0])
    # a device destination: the same draws
    tot, sup, st = e.group_sample_dev(gid, S, d_ids, d_w, None, 0.0, 1, 0)
    host = e.group_sample(gid, S, None, 0.0, 1, 0)
    assert np.array_equal(hip.read(d_ids, 4 * n * S, np.int32).reshape(n, S), host[0]) and np.array_equal(bits(hip.read(d_w, 8 * n * S, np.float64)), bits(host[1]).ravel())
    assert np.array_equal(bits(tot), bits(host[2])) and np.array_equal(sup, host[3]) and np.array_equal(st, host[4])


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_buffer_goes_with_the_engine():
    gc.collect()
    before = eng.live_bytes()
    V0, e1, e2 = datagen.rmat_stream(9, 3000, 11)
    e = eng.Engine(V0 + 5, 600, 1, 20)
    e.load_window(e1[:600], e2[:600])
    gid = e.add_source_group([int(x) for x in datagen.top_sources(V0, e1, e2, 600, 1, 3)])
    e.group_init_solve(gid, EPS)
    held = eng.live_bytes()
    for form in (eng.SAMPLE_WAVE, eng.SAMPLE_PER_THREAD):
        e.debug_sample_form(form)
        ids = e.group_sample(gid, 100)[0]
        assert np.all(ids >= 0)
    assert eng.live_bytes()[0] > held[0] and eng.live_bytes()[1] > held[1]
    e.close()
    assert eng.live_bytes() == before
