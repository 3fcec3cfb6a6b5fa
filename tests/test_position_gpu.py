"""Positions of given vertices in a lane's order (dppr_position_at / dppr_group_position_at) against the numpy restatement of
tests/position_ref.py over what the engine reports through its other calls: the dense columns from group_read / read, the out-CSR of
the epoch by external id from read_out_graph, with the scores of tests/rank_ref.py. Every output is an integer defined by
comparisons alone, so every comparison is array_equal. The anchors of include/dppr.h are proven against the engine's own
group_topk_ranked and group_topk."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import position_ref, rank_ref
from tests.test_dot_gpu import put
from tests.test_export_gpu import Hip
from tests.test_rank_gpu import FLAG_SETS, IN, OUT, S, cols_of, graph_of
from tests.test_renumbering_gpu import churn_stream
from tests.test_weighted_gpu import EPS, Solved, star
from tests.util import small_stream

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 8, 10, 16)
KS = (10, 8192)
MIN_SCORES = (0.0, 1e-4)


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


@pytest.fixture(scope="module", params=[1, 0], ids=["directed", "undirected"])
def solved(request):
    """The engine of tests/test_weighted_gpu.py (small stream, W = 600, c = 20) with one group per width; the anchor test takes its
    look at the init state first, every later test sees the state after two updates (the tests of this module run in file order)."""
    s = Solved(request.param, widths=WIDTHS)
    s.directed = request.param
    s.updates = 0
    yield s
    s.e.close()


def updated(s):
    if s.updates == 0:
        s.update(2)
        s.updates = 2
    return s


def all_ids(e):
    assert e.V <= eng.POSITION_MAX
    return np.arange(e.V, dtype=np.int32)


def check(e, gid, spec, want, what, ids=None, min_scores=MIN_SCORES):
    """group_position_at at `ids` (default: every id) against the reference over the scores `want` (one [V] array per lane)."""
    ids = all_ids(e) if ids is None else np.asarray(ids, dtype=np.int32)
    out = {}
    for ms in min_scores:
        pos, cnt = e.group_position_at(gid, ids, spec, ms)
        wp, wc = position_ref.group_positions(want, ids, ms)
        assert pos.dtype == np.int32 and cnt.dtype == np.int32 and pos.shape == (len(ids), len(want)), what
        assert np.array_equal(cnt, wc), (what, ms, cnt, wc)
        assert np.array_equal(pos, wp), (what, ms, np.argwhere(pos != wp)[:4])
        out[ms] = (pos, cnt)
    return out


def anchors(pos, cnt, ids, lists, k, what):
    """(a) every position below k names its id in the list of the selection; (b) the ids of the list stand at 0, 1, .., in order."""
    where = {int(v): j for j, v in enumerate(ids)}
    for i, (gi, _) in enumerate(lists):
        assert len(gi) == min(k, int(cnt[i])), (what, i, len(gi), cnt[i])
        col = pos[:, i]
        hit = np.nonzero((col >= 0) & (col < k))[0]
        assert np.array_equal(gi[col[hit]], ids[hit]), (what, "a", i)
        rows = np.array([where[int(v)] for v in gi], dtype=np.int64)
        assert np.array_equal(col[rows], np.arange(len(gi), dtype=np.int32)), (what, "b", i)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_anchors_against_the_selections(solved):
    s = solved
    zero = eng.Engine.rank_spec()
    ids = all_ids(s.e)
    for state in ("init", "two updates"):
        if state != "init":
            updated(s)
        for n, gid in s.groups.items():
            cols = cols_of(s.e, gid, n)
            for spec in (None, zero):
                res = check(s.e, gid, spec, cols, (state, n, spec is None))
                for ms in MIN_SCORES:
                    pos, cnt = res[ms]
                    for k in KS:
                        anchors(pos, cnt, ids, s.e.group_topk_ranked(gid, k, ms, spec), k, (state, n, k, ms, "ranked"))
                        if spec is None:  # (c)
                            plain = [(gi, gp) for gi, gp, _ in s.e.group_topk(gid, k, ms)]
                            anchors(pos, cnt, ids, plain, k, (state, n, k, ms, "plain"))
    assert s.updates == 2


def test_a_slot():
    V, e1, e2 = small_stream()
    e = eng.Engine(V, 600, 1, 20)
    e.load_window(e1[:600], e2[:600])
    src = int(datagen.top_sources(V, e1, e2, 600, 1, 1)[0])
    slot = e.add_source(src)
    e.init_solve(slot, EPS)
    p = e.read(slot)[0]
    tails, heads, deg = graph_of(e)
    ids = all_ids(e)
    for spec, want in ((None, p), (eng.Engine.rank_spec(eng.FACTOR_INV_DEG, exclude=S | IN),
                                   rank_ref.scores([p], rank_ref.INV_DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, [[src]], S | IN))[0])):
        for ms in MIN_SCORES:
            pos, cnt = e.position_at(slot, ids, spec, ms)
            wp, wc = position_ref.positions(want, ids, ms)
            assert pos.shape == (V,) and pos.dtype == np.int32 and cnt == wc and np.array_equal(pos, wp)
            for k in KS:
                anchors(pos[:, None], [cnt], ids, [e.topk_ranked(slot, k, ms, spec)], k, ("slot", k, ms))
    assert e.position_at(slot, [src], eng.Engine.rank_spec(exclude=S))[0].tolist() == [-1] and e.position_at(slot, [src])[0].tolist() == [0]
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_whole_order_with_parked_and_unnamed_vertices():
    """m = V = 4096 = DPPR_POSITION_MAX on the churn stream of tests/test_rank_gpu.py, renumbering on: one lane per workgroup."""
    V, W, c, batches = 4096, 1500, 100, 60
    assert V == eng.POSITION_MAX
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
    n_parked = sp["parked"]
    assert n_parked > 0 and sp["renumberings"] > 0, sp
    id_map = e.id_map()
    unnamed = np.nonzero(id_map < 0)[0]
    parked = np.nonzero(id_map >= V - n_parked)[0]
    cols = cols_of(e, gid, 3)
    # the conditions on the fixture: a parked vertex qualifies, a queried id has no internal id
    assert len(unnamed) > 0 and any(np.any(col[parked] > 0) for col in cols)
    tails, heads, deg = graph_of(e)
    ex = rank_ref.excluded(V, tails, heads, [[0], [1], [2]], S | IN | OUT)
    ids = np.arange(V, dtype=np.int32)
    for what, spec, kw in (("plain", None, {}), ("inv_deg", eng.Engine.rank_spec(eng.FACTOR_INV_DEG), dict(factor=rank_ref.INV_DEG, outdeg=deg)),
                           ("deg + all", eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=S | IN | OUT), dict(factor=rank_ref.DEG, outdeg=deg, excl=ex))):
        want = rank_ref.scores(cols, **kw)
        res = check(e, gid, spec, want, ("churn", what), ids)
        for ms, (pos, cnt) in res.items():
            for i in range(3):
                col = pos[:, i]
                assert np.array_equal(np.sort(col[col >= 0]), np.arange(cnt[i])) and np.all(col[col < 0] == -1)   # a permutation and -1s
                assert np.all(col[unnamed] == -1)
            if ms == 0.0:
                assert (pos[parked] >= 0).any()
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_ties_are_cut_by_external_id():
    """The star of tests/test_weighted_gpu.py (both directions stored): the leaves enter in a shuffled order, so the rows are in
    internal order and the ties of p -- and of p times or over a degree -- among them are cut by EXTERNAL id."""
    L = 300
    e, gid, leaves, sources = star(L, lambda lv: [0, int(lv[5]), int(lv[17])])
    cols = cols_of(e, gid, 3)
    tails, heads, deg = graph_of(e)
    id_map = e.id_map()
    assert not np.all(np.diff(id_map[np.sort(leaves)]) > 0)   # internal order is not external order
    for what, spec, kw in (("plain", None, {}), ("deg", eng.Engine.rank_spec(eng.FACTOR_DEG), dict(factor=rank_ref.DEG, outdeg=deg)),
                           ("inv_deg", eng.Engine.rank_spec(eng.FACTOR_INV_DEG), dict(factor=rank_ref.INV_DEG, outdeg=deg))):
        want = rank_ref.scores(cols, **kw)
        for i in range(3):
            q = want[i][want[i] > 0]
            assert len(np.unique(q)) < len(q) - 100, (what, i)   # exact ties, by the hundred
        res = check(e, gid, spec, want, ("star", what), min_scores=(0.0,))
        pos = res[0.0][0]
        tied = np.sort(leaves)
        tied = tied[want[0][tied] == want[0][tied[0]]]
        assert len(tied) > 100 and np.all(np.diff(pos[tied, 0]) == 1)   # equal scores: consecutive positions in id order
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_scores_that_are_not_positive_finite(solved, hip):
    s = updated(solved)
    e, V = s.e, s.V
    rng = np.random.default_rng(21)
    for n in WIDTHS:
        gid = s.groups[n]
        cols = cols_of(e, gid, n)
        top = position_ref.order(cols[0])[:8]
        for dtype, code in ((np.float64, eng.F64), (np.float32, eng.F32)):
            g = (rng.random(V) * 4.0 + 0.01).astype(dtype)
            g[rng.random(V) < 0.1] = 0.0
            g[top[0]], g[top[1]], g[top[2]], g[top[3]], g[top[4]], g[top[5]] = -1.5, np.inf, np.nan, 0.0, np.inf, -np.inf
            spec = eng.Engine.rank_spec(eng.FACTOR_DEV, put(hip, g), code)
            want = rank_ref.scores(cols, rank_ref.DEV, g=g)
            assert np.isnan(want[0]).any() and (want[0] < 0).any() and np.isinf(want[0]).any()
            pos = check(e, gid, spec, want, (s.directed, n, np.dtype(dtype).name))[0.0][0]
            lo, hi = sorted((int(top[1]), int(top[4])))
            assert pos[lo, 0] == 0 and pos[hi, 0] == 1                                    # +inf first, the tie by id
            assert np.all(pos[[top[0], top[2], top[3], top[5]], 0] == -1)                  # negative, NaN, zero, -inf: never
            finite = position_ref.order(np.where(np.isinf(want[0]), 0.0, want[0]))
            assert pos[finite[0], 0] == 2                                                 # ... and nothing of them precedes anything


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_masks_and_per_lane_exclusion(solved, hip):
    s = updated(solved)
    e, V = s.e, s.V
    tails, heads, deg = graph_of(e)
    rng = np.random.default_rng(8)
    half = (rng.random(V) < 0.5).astype(np.uint8)
    d_half = put(hip, half)
    for n in (5, 10, 16):
        gid = s.groups[n]
        cols = cols_of(e, gid, n)
        seeds = [[x] for x in s.srcs[:n]]
        for flags in FLAG_SETS:
            ex = rank_ref.excluded(V, tails, heads, seeds, flags)
            want = rank_ref.scores(cols, excl=ex)
            pos = check(e, gid, eng.Engine.rank_spec(exclude=flags), want, (s.directed, n, flags))[0.0][0]
            both = np.nonzero(ex[2] & ~ex[3] & (want[3] > 0))[0]
            assert len(both) > 0 and np.all(pos[both, 2] == -1) and np.all(pos[both, 3] >= 0)   # out in lane 2, counted in lane 3
        for what, spec, kw in (("allow", eng.Engine.rank_spec(mask=eng.MASK_ALLOW, mask_dev=d_half), dict(allow=half)),
                               ("deny + deg + all", eng.Engine.rank_spec(eng.FACTOR_DEG, mask=eng.MASK_DENY, mask_dev=d_half, exclude=S | IN | OUT),
                                dict(deny=half, factor=rank_ref.DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, seeds, S | IN | OUT)))):
            check(e, gid, spec, rank_ref.scores(cols, **kw), (s.directed, n, what))


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_shapes_tiles_and_pieces(solved):
    s = updated(solved)
    e, V = s.e, s.V
    tails, heads, deg = graph_of(e)
    rng = np.random.default_rng(5)
    spec = eng.Engine.rank_spec(eng.FACTOR_INV_DEG, exclude=S | IN | OUT)
    for n in (1, 10, 16):
        gid = s.groups[n]
        cols = cols_of(e, gid, n)
        want = rank_ref.scores(cols, rank_ref.INV_DEG, outdeg=deg, excl=rank_ref.excluded(V, tails, heads, [[x] for x in s.srcs[:n]], S | IN | OUT))
        best = position_ref.order(want[0])
        # one id; an id four times among others
        check(e, gid, spec, want, (n, "m = 1"), ids=[best[3]])
        dup = np.array([best[7], 3, best[7], best[0], best[7], 3, V - 1, best[7]], dtype=np.int32)
        pos = check(e, gid, spec, want, (n, "duplicates"), ids=dup)[0.0][0]
        assert np.all(pos[[0, 2, 4, 7]] == pos[0]) and pos[0, 0] == 7 and pos[3, 0] == 0 and np.array_equal(pos[1], pos[5])
        # m == 0: the counts alone, or nothing
        pos, cnt = e.group_position_at(gid, np.zeros(0, dtype=np.int32), spec)
        assert pos.shape == (0, n) and np.array_equal(cnt, position_ref.group_positions(want, [], 0.0)[1])
        ip = C.POINTER(C.c_int32)
        assert e._L.dppr_group_position_at(e._h, gid, -1, C.byref(spec), 0.0, None, 0, None, None) == 0
        guard = np.full(n, 77, dtype=np.int32)
        assert e._L.dppr_group_position_at(e._h, gid, -1, C.byref(spec), 0.0, None, 0, None, guard.ctypes.data_as(ip)) == 0
        assert np.array_equal(guard, cnt)
        # 700 ids with repeats: by default several lane blocks of one pass; with a tile of 300 two lane blocks of three passes, with
        # 64, 3 and 1 every lane beside the others and 11, 234 and 700 passes. A piece of 1 entry for the marking beside it.
        many = rng.integers(0, V, 700).astype(np.int32)
        runs = []
        for tile, piece in ((0, 512), (300, 512), (64, 1), (3, 512), (1, 64)):
            e.debug_position_tile(tile)
            e.debug_rank_piece(piece)
            runs.append(check(e, gid, spec, want, (n, "tile", tile, piece), ids=many))
        e.debug_position_tile(0)
        e.debug_rank_piece(512)
        for other in runs[1:]:
            for ms in MIN_SCORES:
                assert np.array_equal(other[ms][0], runs[0][ms][0]) and np.array_equal(other[ms][1], runs[0][ms][1])
    for bad in (-1, 4097):
        with pytest.raises(eng.DpprError):
            e.debug_position_tile(bad)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_on_a_live_engine(hip):
    V, e1, e2 = small_stream()
    W, c = 600, 20
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c, n_epochs=2)
    e.set_renumbering(0)
    e.load_window(*g.window_edges())
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, 1, 2)]
    gid = e.add_source_group(srcs)
    slot = e.add_source(srcs[0])
    e.group_init_solve(gid, EPS)
    e.init_solve(slot, EPS)
    newest = 0
    for _ in range(2):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        newest = e.slide(*g.new_stream())
        e.group_update(gid, EPS)
        e.update(slot, EPS)
    L, h = e._L, e._h
    ip = C.POINTER(C.c_int32)
    M = 8
    pos, cnt = np.full(2 * M, 77, dtype=np.int32), np.full(2, 99, dtype=np.int32)
    P, N = pos.ctypes.data_as(ip), cnt.ctypes.data_as(ip)
    at = np.arange(M, dtype=np.int32)
    A = at.ctypes.data_as(ip)

    def refused(spec=None, epoch=-1, ms=0.0, ids=A, m=M, out=P, counts=N, group=gid, slot_=slot):
        sp = C.byref(spec) if spec is not None else None
        rcs = (L.dppr_group_position_at(h, group, epoch, sp, ms, ids, m, out, counts), L.dppr_position_at(h, slot_, epoch, sp, ms, ids, m, out, counts))
        return rcs == (-1, -1) and bool(np.all(pos == 77) and np.all(cnt == 99))

    spec = eng.Engine.rank_spec
    g64 = np.ones(V)
    d_g = put(hip, g64)
    d_mask = put(hip, np.zeros(V, dtype=np.uint8))
    big = np.zeros(eng.POSITION_MAX + 1, dtype=np.int32)
    for kw in (dict(m=-1), dict(ids=big.ctypes.data_as(ip), m=eng.POSITION_MAX + 1), dict(ids=None), dict(out=None), dict(ms=-1e-300),
               dict(ms=float("nan")), dict(ids=np.array([0, -1] * 4, dtype=np.int32).ctypes.data_as(ip)),
               dict(ids=np.array([V, 0] * 4, dtype=np.int32).ctypes.data_as(ip)), dict(group=5, slot_=5), dict(group=-1, slot_=-1)):
        assert refused(**kw), list(kw)
    # every spec rejection of dppr_topk_ranked
    for sp in (spec(eng.FACTOR_DEV, g64.ctypes.data), spec(eng.FACTOR_DEV, 0), spec(eng.FACTOR_DEV, put(hip, np.ones(V - 1))),
               spec(eng.FACTOR_DEV, d_g + 4), spec(eng.FACTOR_DEV, d_g, 2), spec(mask=eng.MASK_ALLOW, mask_dev=g64.ctypes.data),
               spec(mask=eng.MASK_DENY, mask_dev=d_mask + 1), spec(4), spec(-1), spec(mask=3), spec(exclude=8)):
        assert refused(sp), (sp.factor, sp.factor_dtype, sp.mask, sp.exclude)
    # ... and every epoch rejection, where the spec needs one; the epoch is not looked at where it does not
    e.read_out_graph(newest - 1)  # (resident)
    for sp in (spec(eng.FACTOR_DEG), spec(eng.FACTOR_INV_DEG), spec(exclude=IN), spec(exclude=OUT)):
        assert refused(sp, newest - 1) and b"another epoch" in L.dppr_last_error(h)
        assert refused(sp, newest - 2) and refused(sp, newest + 1) and b"not resident" in L.dppr_last_error(h)
    cols = cols_of(e, gid, 2)
    for sp in (None, spec(), spec(eng.FACTOR_DEV, d_g), spec(mask=eng.MASK_DENY, mask_dev=d_mask)):
        got = e.group_position_at(gid, at, sp, epoch=newest + 5)
        want = position_ref.group_positions(cols, at)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the limits themselves are accepted, and a valid call writes exactly the documented shape
    assert len(e.group_position_at(gid, big[:eng.POSITION_MAX])[0]) == eng.POSITION_MAX
    assert L.dppr_group_position_at(h, gid, -1, None, 0.0, A, M - 1, P, None) == 0
    assert np.array_equal(pos[:2 * (M - 1)].reshape(M - 1, 2), position_ref.group_positions(cols, at[:M - 1])[0]) and np.all(pos[2 * (M - 1):] == 77)
    assert np.all(cnt == 99)
    e.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_after_another_family_and_every_buffer_goes_with_the_engine():
    """group_topk_weighted and group_changes run first on one engine, so the shared scratch state is already there (two planes, 16
    lanes wide); the result equals a fresh engine's, and all of it goes with the engine."""
    gc.collect()
    before = eng.live_bytes()
    results = []
    for warm in (True, False):
        s = Solved(1, widths=(10,))
        gid = s.groups[10]
        if warm:
            s.e.group_mark(gid)
        s.update(2)
        if warm:
            s.e.group_topk_weighted(gid, np.ones((16, 10)), 100, 0.0)
            s.e.group_changes(gid, 100, 0.0)
        held = eng.live_bytes()
        spec = eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=S | IN | OUT)
        results.append(s.e.group_position_at(gid, all_ids(s.e), spec))
        assert eng.live_bytes()[0] > held[0]   # (keys, slots and the block are there)
        s.e.close()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1]) and results[0][1].min() > 0
    assert eng.live_bytes() == before
