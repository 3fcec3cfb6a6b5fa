"""The ranked, position and sample queries over a forward track (dppr_ftrack_topk_ranked / _rank_score_at / _position_at / _sample) on
the device against numpy (tests/ftrack_rank_ref.py over tests/rank_ref.py, tests/position_ref.py and tests/sample_ref.py): the track's
columns by external id from tests/ftrack_ref.py (RefTrack), the epoch's out-rows from dppr_read_out_graph, the seeds as the external
ids of the start sets. No tolerance appears anywhere: ids, counts, positions and statuses are compared as integers, scores, weights
and totals by bit pattern. The fixtures are those of tests/test_ftrack_gpu.py: the R-MAT scale-10 stream, V = 1024, 4000 window
edges, 50-edge batches."""
import ctypes as C

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from tests import ftrack_rank_ref as frr
from tests.test_dot_gpu import put
from tests.test_export_gpu import Hip
from tests.test_forward_gpu import bits, rows_of, star
from tests.test_fpush_gpu import as_set
from tests.test_ftrack_gpu import RefTrack, Window, standard_sets
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

S, IN, OUT = eng.EXCLUDE_SEEDS, eng.EXCLUDE_IN_NEIGHBOURS, eng.EXCLUDE_OUT_NEIGHBOURS
FLAG_SETS = (S, IN, OUT, S | IN | OUT)   # (those of tests/test_rank_gpu.py)
KS, MIN_SCORES = (10, 8192), (0.0, 1e-4)


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def graph_of(e, epoch=-1):
    row, col = e.read_out_graph(epoch)
    return frr.Graph(e.V, row, col)


def seeds_of(sets):
    return [as_set(s)[0] for s in sets]


def spec_cases(hip, V, rng):
    """(name, the spec, the reference's arguments): every factor (DEV in f64 and f32 with negative and zero entries), both masks, the
    four flag sets, and all of it together."""
    cases = [("null", None, {}), ("zero", eng.Engine.rank_spec(), {}),
             ("deg", eng.Engine.rank_spec(eng.FACTOR_DEG), dict(factor=frr.DEG)),
             ("inv_deg", eng.Engine.rank_spec(eng.FACTOR_INV_DEG), dict(factor=frr.INV_DEG))]
    for dtype, code in ((np.float64, eng.F64), (np.float32, eng.F32)):
        g = (rng.random(V) * 4.0 - 1.0).astype(dtype)   # (a quarter is negative)
        g[rng.random(V) < 0.1] = 0.0
        cases.append((f"dev {np.dtype(dtype).name}", eng.Engine.rank_spec(eng.FACTOR_DEV, put(hip, g), code), dict(factor=frr.DEV, g=g)))
    allow = (rng.random(V) < 0.5).astype(np.uint8) * 3
    deny = (rng.random(V) < 0.3).astype(np.uint8)
    cases.append(("allow", eng.Engine.rank_spec(mask=eng.MASK_ALLOW, mask_dev=put(hip, allow)), dict(allow=allow)))
    cases.append(("deny", eng.Engine.rank_spec(mask=eng.MASK_DENY, mask_dev=put(hip, deny)), dict(deny=deny)))
    for f in FLAG_SETS:
        cases.append((f"exclude {f}", eng.Engine.rank_spec(exclude=f), dict(exclude=f)))
    cases.append(("all", eng.Engine.rank_spec(eng.FACTOR_INV_DEG, mask=eng.MASK_DENY, mask_dev=put(hip, deny), exclude=S | IN | OUT),
                  dict(factor=frr.INV_DEG, deny=deny, exclude=S | IN | OUT)))
    return cases


def same_topk(got, want, k, ms, what):
    assert len(got) == len(want), what
    for i, (gi, gs) in enumerate(got):
        wi, ws = frr.topk(want[i], k, ms)
        assert np.array_equal(gi, wi), (what, i, k, ms, gi[:8], wi[:8], len(gi), len(wi))
        assert np.array_equal(bits(gs), bits(ws)), (what, i, k, ms)


def check(t, want, spec, what, ks=KS, min_scores=MIN_SCORES):
    """topk_ranked at every k and min_score and rank_score_at at all V ids against the reference scores `want` (one [V] array per
    column of the track)."""
    m, V = len(want), len(want[0])
    for k in ks:
        for ms in min_scores:
            same_topk(t.topk_ranked(k, ms, spec), want, k, ms, what)
    dense = t.rank_score_at(np.arange(V, dtype=np.int32), spec)
    assert dense.shape == (V, m)
    for i in range(m):
        assert np.array_equal(bits(dense[:, i]), bits(want[i])), (what, "score_at", i)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_definition_after_the_create_and_after_every_batch(directed, hip):
    w = Window(directed)
    e, V = w.e, w.V
    sets, who = standard_sets(w)
    seeds = seeds_of(sets)
    cases = spec_cases(hip, V, np.random.default_rng(5))
    refs = {"converged": RefTrack(w.rows, sets, 1e-6, 64), "five rounds": RefTrack(w.rows, sets, 1e-8, 5)}
    tracks = [("converged", m, e.ftrack(sets[:m], 1e-6, 64)) for m in (1, 5, 16)] + [("five rounds", 16, e.ftrack(sets, 1e-8, 5))]
    negative = 0
    unnamed = who["unnamed"]
    assert np.array_equal(seeds[2], [unnamed]) and e.id_map()[unnamed] < 0   # column 2: its only seed has no row
    for b in range(7):
        if b:
            rec, rows = w.slide()
            for ref in refs.values():
                ref.update(rows, rec, 64 if ref is refs["converged"] else 5)
            for name, _, t in tracks:
                t.update(w.epoch, 64 if name == "converged" else 5)
            negative += int(any(np.any(c.p < 0) for c in refs["converged"].cols))
        graph = graph_of(e)
        for name, ref in refs.items():
            cols = [c.p for c in ref.cols]
            for what, spec, kw in cases:
                want = frr.scores(cols, seeds, graph, **kw)   # (once per epoch, state and spec: the widths are prefixes of it)
                for tname, m, t in tracks:
                    if tname == name:
                        check(t, want[:m], spec, (directed, b, name, m, what))
        # the vertex the stream never names: first (and alone) in its own column's raw order, gone under EXCLUDE_SEEDS, although it has no row
        t16 = tracks[2][2]
        raw, gone = t16.topk_ranked(10)[2], t16.topk_ranked(10, spec=eng.Engine.rank_spec(exclude=S))[2]
        assert raw[0].tolist() == [unnamed] and raw[1][0] == 0.15 and len(gone[0]) == 0, (b, raw, gone)
        big = t16.topk_ranked(8192)[4][0]
        assert unnamed in big and unnamed not in t16.topk_ranked(8192, spec=eng.Engine.rank_spec(exclude=S))[4][0]
    assert negative > 0   # some batch made some p negative: such a score never qualifies
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_anchors_against_ftrack_read_and_ftrack_cluster(directed):
    w = Window(directed)
    e, V = w.e, w.V
    sets, who = standard_sets(w)
    t = e.ftrack(sets, 1e-6, 64)
    no_rowless = [sets[i] for i in (0, 1, 3, 5)]   # hub, sink, the two-seed set, the median-degree vertex: every seed has a row
    tc = e.ftrack(no_rowless, 1e-6, 64)
    compared = 0
    for b in range(4):
        if b:
            w.slide()
            t.update(w.epoch, 64)
            tc.update(w.epoch, 64)
        for k in (10, 8192):
            for ms in (0.0, 1e-4):
                plain = t.read(k=k, min_p=ms)["topk"]
                for spec in (None, eng.Engine.rank_spec()):
                    got = t.topk_ranked(k, ms, spec)
                    assert len(got) == len(plain) == 16
                    for i in range(16):   # (a): column 2's only seed is rowless
                        assert np.array_equal(got[i][0], plain[i][0]) and np.array_equal(bits(got[i][1]), bits(plain[i][1])), (b, k, ms, i)
                        if k == 10 and len(got[i][0]):   # (b)
                            assert np.array_equal(bits(t.rank_score_at(got[i][0], spec)[:, i]), bits(got[i][1])), (b, ms, i)
        assert t.topk_ranked(10)[2][0].tolist() == [who["unnamed"]]
        # (c): INV_DEG and nothing else against the conductance sweep's order by p / (outdeg + 1): a selection against a radix sort.
        # The sweep orders the vertices an edge names; a column is compared where every vertex with a positive score is named
        # (always on a fresh track: p > 0 is reached over an edge).
        graph = graph_of(e)
        named = (graph.outdeg > 0) | (np.bincount(graph.heads, minlength=V) > 0)
        at_p = tc.read(at=np.arange(V, dtype=np.int32))["at_p"]
        inv = eng.Engine.rank_spec(eng.FACTOR_INV_DEG)
        for k in (10, 8192):
            for ms in (0.0, 1e-6):
                got = tc.topk_ranked(k, ms, inv)
                _, off, ids, score = tc.cluster("deg", min_score=ms, max_len=k if k <= V else 0, profile=True)[:4]
                for i in range(len(no_rowless)):
                    if b and np.any((at_p[i] > 0) & ~named):
                        continue
                    assert np.array_equal(got[i][0], ids[off[i]:off[i + 1]]) and np.array_equal(bits(got[i][1]), bits(score[off[i]:off[i + 1]])), (b, k, ms, i)
                    compared += 1
    assert compared >= 4 * 4 + 4   # every column on the fresh track, and some after a batch
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_exclusion_is_per_column():
    w = Window(1)
    e, V = w.e, w.V
    sets, who = standard_sets(w)
    pair = [sets[4], who["hub"]]   # the 64-seed set and the hub share a track
    t, ref = e.ftrack(pair, 1e-6, 64), RefTrack(w.rows, pair, 1e-6, 64)
    rec, rows = w.slide()
    ref.update(rows, rec, 64)
    t.update(w.epoch, 64)
    graph, seeds, cols = graph_of(e), seeds_of(pair), [c.p for c in ref.cols]
    flags = S | IN | OUT
    spec = eng.Engine.rank_spec(exclude=flags)
    want = frr.scores(cols, seeds, graph, exclude=flags)
    check(t, want, spec, "per column")
    top = t.topk_ranked(8192, 0.0, spec)
    only0 = [v for v in range(V) if want[0][v] == 0.0 and cols[0][v] > 0 and want[1][v] > 0]   # excluded in column 0, ranked in column 1
    only1 = [v for v in range(V) if want[1][v] == 0.0 and cols[1][v] > 0 and want[0][v] > 0]
    assert only0 and only1
    assert all(v not in top[0][0] and v in top[1][0] for v in only0) and all(v not in top[1][0] and v in top[0][0] for v in only1)
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_hub_rows_in_pieces_ties_and_every_tile_setting():
    """The star of tests/test_forward_gpu.py with D = 1500 > 512: from the start S (out-degree D) every leaf of equal out-degree ties,
    the head 0 has in-degree D. The columns are the track's own p as dppr_ftrack_read reports it. Every dppr_debug_rank_piece /
    dppr_debug_ftrack_rank setting gives one blob of bits, and the blob is numpy's."""
    D = 1500
    V, tails, heads, start = star(D)
    e = eng.Engine(V, len(tails), 1, 1)
    e.load_window(tails, heads)
    sink = V - 1   # a vertex with in-edges only
    sets = [start, 0, (np.array([start, 3]), np.array([2.0, 0.5])), sink]
    t = e.ftrack(sets, 1e-5, 3)
    at = np.arange(V, dtype=np.int32)
    cols = list(t.read(at=at)["at_p"])
    graph, seeds = graph_of(e), seeds_of(sets)
    assert graph.outdeg[start] == D and np.bincount(graph.heads, minlength=V)[0] == D
    leaves = cols[0][1:D + 1]
    tie = np.unique(leaves[np.arange(1, D + 1) % 5 == 0])
    assert len(tie) == 1 and tie[0] > 0 and np.count_nonzero(leaves == tie[0]) > 512   # a tie longer than a piece and than a tile
    order0 = frr.topk(cols[0], 8192)[0]
    tied = order0[np.isin(order0, np.nonzero(cols[0] == tie[0])[0])]
    assert np.all(np.diff(tied) > 0)   # ties stand in ascending external id
    only_start = float(np.sort(np.unique(cols[0]))[-2])   # strict: nothing but the largest entry of column 0 is above it
    specs = [("null", None, {}), ("out", eng.Engine.rank_spec(exclude=OUT), dict(exclude=OUT)),
             ("in", eng.Engine.rank_spec(eng.FACTOR_INV_DEG, exclude=S | IN), dict(factor=frr.INV_DEG, exclude=S | IN)),
             ("all", eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=S | IN | OUT), dict(factor=frr.DEG, exclude=S | IN | OUT))]
    dup = np.concatenate([at, at[:7], [start, 0, 5, 5]]).astype(np.int32)
    first = None
    for piece in (1, 64, 512):
        e.debug_rank_piece(piece)
        for tile in (0, 64, 1024):
            e.debug_ftrack_rank(tile)
            blob = []
            for what, spec, kw in specs:
                want = frr.scores(cols, seeds, graph, **kw) if first is None else None
                for ms in (0.0, only_start, 10.0):   # every tile keeps rows | most tiles keep none | no row is kept at all
                    got = t.topk_ranked(8192, ms, spec)
                    pos, cnt = t.position_at(dup, spec, ms)
                    blob += [np.concatenate([g[0] for g in got]).tobytes(), np.concatenate([g[1] for g in got]).tobytes(), pos.tobytes(), cnt.tobytes()]
                    if want is not None:
                        same_topk(got, want, 8192, ms, (what, ms))
                        wpos, wcnt = frr.positions(want, dup, ms)
                        assert np.array_equal(pos, wpos) and np.array_equal(cnt, wcnt), (what, ms)
                        if ms == 10.0:
                            assert cnt.tolist() == [0, 0, 0, 0] and np.all(pos == -1) and all(len(g[0]) == 0 for g in got)
                        if ms == only_start and what == "null":
                            assert cnt[0] == 1 and len(got[0][0]) == 1 and got[0][0][0] == start   # one kept row of column 0: most tiles keep none
                        if ms == 0.0 and what == "in":
                            assert cnt[3] == 0 and cnt[0] > 512   # column 3 holds p at its seed alone: a whole column without a kept row
                blob.append(t.rank_score_at(at, spec).tobytes())
                if want is not None:
                    assert np.array_equal(bits(t.rank_score_at(at, spec)), bits(np.stack(want, axis=1))), what
            first = blob if first is None else first
            assert blob == first, (piece, tile)
    assert only_start < cols[0][start] and cols[3][sink] == 0.15 and np.count_nonzero(cols[3]) == 1
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_positions(directed, hip):
    w = Window(directed)
    e, V = w.e, w.V
    sets, who = standard_sets(w)
    seeds = seeds_of(sets)
    t, ref = e.ftrack(sets, 1e-6, 64), RefTrack(w.rows, sets, 1e-6, 64)
    for _ in range(2):
        rec, rows = w.slide()
        ref.update(rows, rec, 64)
        t.update(w.epoch, 64)
    graph, cols = graph_of(e), [c.p for c in ref.cols]
    rng = np.random.default_rng(9)
    ids = np.concatenate([rng.permutation(V), rng.integers(0, V, 40), [who["unnamed"], who["unnamed"], who["hub"]]]).astype(np.int32)
    cases = [c for c in spec_cases(hip, V, rng) if c[0] in ("null", "deg", "dev float32", "allow", "exclude 7", "all")]
    first = {}
    for tile in (0, 1, 64):
        e.debug_position_tile(tile)
        for what, spec, kw in cases:
            if tile == 1 and what not in ("null", "all"):
                continue
            want = frr.scores(cols, seeds, graph, **kw)
            for ms in MIN_SCORES:
                pos, cnt = t.position_at(ids, spec, ms)
                wpos, wcnt = frr.positions(want, ids, ms)
                assert pos.shape == (len(ids), 16) and np.array_equal(pos, wpos) and np.array_equal(cnt, wcnt), (directed, tile, what, ms)
                assert (pos.tobytes(), cnt.tobytes()) == first.setdefault((what, ms), (pos.tobytes(), cnt.tobytes()))
                if tile == 0:   # anchors (d), against dppr_ftrack_topk_ranked
                    top = t.topk_ranked(50, ms, spec)
                    for i, (ti, _) in enumerate(top):
                        inside = (pos[:, i] >= 0) & (pos[:, i] < 50)
                        assert np.array_equal(ti[pos[inside, i]], ids[inside]), (what, ms, i)                       # (a)
                        if len(ti):
                            assert t.position_at(ti, spec, ms)[0][:, i].tolist() == list(range(len(ti))), (what, ms, i)   # (b)
    pos, cnt = t.position_at(np.zeros(0, dtype=np.int32))
    assert pos.shape == (0, 16) and np.array_equal(cnt, frr.positions(cols, [], 0.0)[1])   # n_ids == 0: the counts alone
    mrr, hits = eng.rank_metrics(t.position_at(ids[:V])[0][:, 0], (1, 10))
    assert 0.0 < mrr <= 1.0 and hits[1] == 1.0 / V   # rank_metrics takes a column of positions
    e.debug_position_tile(0)
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_samples(directed, hip):
    w = Window(directed)
    e, V = w.e, w.V
    sets, who = standard_sets(w)
    seeds = seeds_of(sets)
    t, ref = e.ftrack(sets, 1e-6, 64), RefTrack(w.rows, sets, 1e-6, 64)
    rec, rows = w.slide()
    ref.update(rows, rec, 64)
    t.update(w.epoch, 64)
    graph, cols = graph_of(e), [c.p for c in ref.cols]
    NS, FIRST, SEED = 257, 2 ** 32 - 5, 0xC0FFEE1234
    rng = np.random.default_rng(13)
    cases = [c for c in spec_cases(hip, V, rng) if c[0] in ("null", "inv_deg", "dev float64", "deny", "exclude 1", "all")]
    d_ids, d_w = hip.alloc(4 * 16 * NS), hip.alloc(8 * 16 * NS)
    for what, spec, kw in cases:
        want_scores = frr.scores(cols, seeds, graph, **kw)
        for ms in MIN_SCORES:
            want = frr.sample(want_scores, NS, ms, SEED, FIRST)
            results = []
            for form in (eng.SAMPLE_WAVE, eng.SAMPLE_PER_THREAD):
                e.debug_sample_form(form)
                ids, wt, total, support, status = t.sample(NS, spec, ms, SEED, FIRST)
                assert np.array_equal(ids, want[0]) and np.array_equal(bits(wt), bits(want[1])), (directed, what, ms, form)
                assert np.array_equal(bits(total), bits(want[2])) and np.array_equal(support, want[3]) and np.array_equal(status, want[4]), (what, ms, form)
                tot2, sup2, st2 = t.sample(NS, spec, ms, SEED, FIRST, device_ptrs=dict(ids=d_ids, w=d_w))   # a device destination
                assert np.array_equal(hip.read(d_ids, 4 * 16 * NS).view(np.int32).reshape(16, NS), ids)
                assert np.array_equal(hip.read(d_w, 8 * 16 * NS).view(np.uint64).reshape(16, NS), bits(wt))
                assert np.array_equal(bits(tot2), bits(total)) and np.array_equal(sup2, support) and np.array_equal(st2, status)
                results.append((ids, wt))
            e.debug_sample_form(eng.SAMPLE_WAVE)
            ids, wt = results[0]
            # anchors (e)
            back = t.rank_score_at(np.where(ids < 0, 0, ids).ravel(), spec).reshape(16, NS, 16)
            for i in range(16):
                if status[i] == eng.SAMPLE_OK:
                    assert np.array_equal(bits(back[i, :, i]), bits(wt[i])) and np.all(wt[i] > ms), (what, ms, i)   # (a)
                else:
                    assert np.all(ids[i] == -1) and np.all(bits(wt[i]) == 0)
            a = t.sample(100, spec, ms, SEED, FIRST, with_w=False)[0]
            z = t.sample(NS - 100, spec, ms, SEED, FIRST + 100, with_w=False)[0]
            assert np.array_equal(np.concatenate([a, z], axis=1), ids), (what, ms)                                       # (b)
            none = t.sample(0, spec, ms, SEED, FIRST)
            assert none[0].shape == (16, 0) and np.array_equal(bits(none[2]), bits(total)) and np.array_equal(none[4], status)   # (d)
            if what == "null":       # (c) column 2: one positive leaf, the vertex the stream never names
                assert support[2] == 1 and np.all(ids[2] == who["unnamed"]) and total[2] == 0.15
            if what == "exclude 1":  # ... and EMPTY once its only seed is excluded
                assert status[2] == eng.SAMPLE_EMPTY and support[2] == 0 and np.all(ids[2] == -1)
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_after_a_renumbering_slide(hip):
    """The window of test_a_track_follows_a_renumbering: vertices are parked and revived, the internal ids move. The track's state and
    the exclusion words are by external id: the results still equal the reference."""
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    w = Window(1, V=V, e1=e1, e2=e2, Wn=W, c=c, renumbering=dict(growth_pct=10, min_parked=16))
    e = w.e
    gid = e.add_source_group([0, 1, 2])   # (a solver that follows the stream, as in test_a_track_follows_a_renumbering)
    e.group_init_solve(gid, 1e-9)
    rows = rows_of(e)
    w.rows = rows
    named = np.nonzero((e.id_map() >= 0) & (rows.d > 0))[0]
    sets = [int(named[0]), (named[[3, 50, 200]], np.array([1.0, 0.7, 2.0])), int(np.argmax(rows.d)), int(named[-1]),
            (named[5:69], 0.5 + np.arange(64) / 64.0)]
    seeds = seeds_of(sets)
    t, ref = e.ftrack(sets, 1e-6, 64), RefTrack(rows, sets, 1e-6, 64)
    cases = [c for c in spec_cases(hip, V, np.random.default_rng(3)) if c[0] in ("null", "deg", "exclude 7", "all")]
    r0 = e.id_space()["renumberings"]
    ids = np.random.default_rng(4).permutation(V)[:1000].astype(np.int32)
    parked_with_p = 0
    for b in range(batches):
        rec, rows = w.slide()
        e.group_update(gid, 1e-9)
        ref.update(rows, rec, 64)
        t.update(w.epoch, 64)
        cols = [c.p for c in ref.cols]
        x2i, sp = e.id_map(), e.id_space()
        parked_now = bool(np.any((x2i >= V - sp["parked"]) & (np.stack(cols).max(axis=0) > 0)))
        parked_with_p += int(parked_now)
        if b % 10 != 9 and not (parked_now and parked_with_p == 1):
            continue
        graph = graph_of(e)
        for what, spec, kw in cases:
            want = frr.scores(cols, seeds, graph, **kw)
            check(t, want, spec, ("churn", b, what), ks=(10, 8192), min_scores=(0.0,))
            pos, cnt = t.position_at(ids, spec)
            wpos, wcnt = frr.positions(want, ids)
            assert np.array_equal(pos, wpos) and np.array_equal(cnt, wcnt), (b, what)
        got = t.sample(65, cases[3][1], 0.0, 7, 11)
        ws = frr.sample(frr.scores(cols, seeds, graph, **cases[3][2]), 65, 0.0, 7, 11)
        assert np.array_equal(got[0], ws[0]) and np.array_equal(bits(got[1]), bits(ws[1])) and np.array_equal(bits(got[2]), bits(ws[2]))
    sp = e.id_space()
    assert sp["renumberings"] > r0 and sp["parked"] > 0 and parked_with_p > 0, (sp, parked_with_p)   # a parked vertex keeps its value and its place
    e.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_track_and_the_outputs_untouched(hip):
    w = Window(1, n_epochs=2)
    e, V = w.e, w.V
    L, h = e._L, e._h
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    sets = [1, (np.array([2, 5]), np.array([0.5, 2.0]))]
    t = e.ftrack(sets, 1e-6, 8)
    at = np.arange(V, dtype=np.int32)
    state = t.read(at=at)
    ints, dbls = np.full(4096 * 2 + 64, 77, dtype=np.int32), np.full(4096 * 2 + 64, 7.5)
    ids = np.array([1, 2, V - 1], dtype=np.int32)
    d_g, d_mask = hip.alloc(8 * V), hip.alloc(V)
    d_ids, d_w = hip.alloc(4 * 2 * 16), hip.alloc(8 * 2 * 16)
    I, D = ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp)

    def unchanged():
        now = t.read(at=at)
        return bool(np.all(ints == 77) and np.all(dbls == 7.5) and np.all(hip.read(d_ids, 4 * 2 * 16) == 0xAB) and np.all(hip.read(d_w, 8 * 2 * 16) == 0xAB)
                    and all(np.asarray(now[x]).tobytes() == np.asarray(state[x]).tobytes() for x in state))

    def refused(rc, words):
        return rc == -1 and unchanged() and words.encode() in L.dppr_last_error(h)

    def topk(track=None, spec=None, k=4, ms=0.0, o_ids=I, o_sc=D, o_cnt=I):
        return L.dppr_ftrack_topk_ranked(h, t.handle if track is None else track, C.byref(spec) if spec is not None else None, k, ms, o_ids, o_sc, o_cnt)

    def score_at(track=None, spec=None, q=ids, n=None, out=D):
        return L.dppr_ftrack_rank_score_at(h, t.handle if track is None else track, C.byref(spec) if spec is not None else None,
                                           None if q is None else q.ctypes.data_as(ip), len(q) if n is None else n, out)

    def position(track=None, spec=None, ms=0.0, q=ids, n=None, pos=I, cnt=I):
        return L.dppr_ftrack_position_at(h, t.handle if track is None else track, C.byref(spec) if spec is not None else None, ms,
                                         None if q is None else q.ctypes.data_as(ip), len(q) if n is None else n, pos, cnt)

    def sample(track=None, spec=None, ms=0.0, first=0, n=4, dest=eng.DEST_HOST, o_ids="host", o_w="host", total=D, status=I):
        o_ids = ints.ctypes.data if o_ids == "host" else o_ids
        o_w = dbls.ctypes.data if o_w == "host" else o_w
        return L.dppr_ftrack_sample(h, t.handle if track is None else track, C.byref(spec) if spec is not None else None, ms, 3, first, n, dest, o_ids, o_w,
                                    total, I, status)

    rs = eng.Engine.rank_spec
    bad_specs = [rs(factor=4), rs(factor=-1), rs(eng.FACTOR_DEV, d_g, 2), rs(mask=3), rs(mask=-1), rs(exclude=8), rs(exclude=16 | S),
                 rs(eng.FACTOR_DEV, 0), rs(eng.FACTOR_DEV, d_g + 4), rs(eng.FACTOR_DEV, ints.ctypes.data), rs(eng.FACTOR_DEV, d_mask),   # (V bytes: too short)
                 rs(mask=eng.MASK_ALLOW, mask_dev=0), rs(mask=eng.MASK_DENY, mask_dev=ints.ctypes.data), rs(mask=eng.MASK_ALLOW, mask_dev=d_mask + 1)]
    for spec in bad_specs:
        assert refused(topk(spec=spec), "") and refused(score_at(spec=spec), "") and refused(position(spec=spec), "") and refused(sample(spec=spec), "")
    for track in (-1, 16, t.handle + 1):
        assert refused(topk(track=track), "no such track") and refused(score_at(track=track), "no such track")
        assert refused(position(track=track), "no such track") and refused(sample(track=track), "no such track")
    nan = float("nan")
    assert refused(topk(k=0), "k in [1") and refused(topk(k=8193), "k in [1") and refused(topk(ms=-1.0), "min_score") and refused(topk(ms=nan), "min_score")
    assert refused(topk(o_ids=None), "non-null") and refused(topk(o_sc=None), "non-null") and refused(topk(o_cnt=None), "non-null")
    bad_id, neg_id = np.array([1, V], dtype=np.int32), np.array([-1, 2], dtype=np.int32)
    assert refused(score_at(n=-1), "ids in [0, V)") and refused(score_at(q=bad_id), "ids in [0, V)") and refused(score_at(q=neg_id), "ids in [0, V)")
    assert refused(score_at(q=None, n=3), "ids in [0, V)") and refused(score_at(out=None), "non-null score")
    many = np.zeros(eng.POSITION_MAX + 1, dtype=np.int32)
    assert refused(position(n=-1), "n_ids in [0") and refused(position(q=many), "n_ids in [0") and refused(position(q=bad_id), "ids in [0, V)")
    assert refused(position(ms=-0.5), "min_score") and refused(position(ms=nan), "min_score") and refused(position(q=None, n=2), "non-null")
    assert refused(position(pos=None), "non-null")
    assert refused(sample(n=-1), "S in [0") and refused(sample(n=eng.SAMPLE_MAX + 1), "S in [0") and refused(sample(first=2 ** 64 - 2), "without a wrap")
    assert refused(sample(dest=2), "dest 0 or 1") and refused(sample(ms=-1.0), "min_score") and refused(sample(ms=nan), "min_score")
    assert refused(sample(o_ids=None), "non-null ids") and refused(sample(total=None), "non-null total") and refused(sample(status=None), "non-null total")
    assert refused(sample(dest=eng.DEST_DEVICE, o_ids=ints.ctypes.data, o_w=None), "a device destination")
    assert refused(sample(dest=eng.DEST_DEVICE, o_ids=d_ids + 2, o_w=None), "a device destination")
    assert refused(sample(dest=eng.DEST_DEVICE, o_ids=d_ids, o_w=d_w + 4), "a device destination")
    assert refused(sample(dest=eng.DEST_DEVICE, n=17, o_ids=d_ids, o_w=None), "a device destination")   # 2 x 17 draws: beyond the allocation
    # (m * S <= DPPR_SAMPLE_MAX_TOTAL binds at m = 16: a 16-column track, S = 2^20 + 0 is the limit itself; one more is S's own limit)
    assert L.dppr_debug_ftrack_rank(h, 32) == -1 and L.dppr_debug_ftrack_rank(h, 96) == -1 and L.dppr_debug_ftrack_rank(h, 2048) == -1
    assert L.dppr_debug_ftrack_rank(h, 128) == 0 and L.dppr_debug_ftrack_rank(h, 0) == 0
    # n_ids == 0 and S == 0 behave as in the group forms
    assert score_at(q=ids, n=0) == 0 and position(q=ids, n=0, cnt=None) == 0 and unchanged()
    # the epoch rule: a spec without degrees or neighbours still answers after the track's epoch has left the ring; one with is refused
    plain_specs = (None, rs(), rs(exclude=S), rs(eng.FACTOR_DEV, put(hip, np.ones(V))), rs(mask=eng.MASK_DENY, mask_dev=put(hip, np.zeros(V, dtype=np.uint8))))
    before = [t.topk_ranked(10, 0.0, sp) for sp in plain_specs]
    w.slide()
    w.slide()   # epochs 1 and 2 are resident (n_epochs = 2), the track's epoch 0 is not
    for sp, was in zip(plain_specs, before):
        now = t.topk_ranked(10, 0.0, sp)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) for a, b in zip(now, was))
        assert t.rank_score_at(ids, sp).shape == (3, 2) and t.position_at(ids, sp)[0].shape == (3, 2) and t.sample(5, sp)[0].shape == (2, 5)
    for sp in (rs(eng.FACTOR_DEG), rs(eng.FACTOR_INV_DEG), rs(exclude=IN), rs(exclude=S | OUT)):
        assert refused(topk(spec=sp), "no longer resident") and refused(score_at(spec=sp), "no longer resident")
        assert refused(position(spec=sp), "no longer resident") and refused(sample(spec=sp), "no longer resident")
    gone = t.handle
    t.close()
    assert L.dppr_ftrack_topk_ranked(h, gone, None, 4, 0.0, I, D, I) == -1 and np.all(ints == 77) and np.all(dbls == 7.5)
    e.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_buffer_goes_with_the_engine_and_the_scratch_is_shared():
    base = eng.live_bytes()
    w = Window(1)
    e, V = w.e, w.V
    sets, who = standard_sets(w)
    srcs = [who["hub"], who["med"], 1]
    gid = e.add_source_group(srcs)
    e.group_init_solve(gid, 1e-8)
    t = e.ftrack(sets, 1e-6, 64)
    gspec = eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=S | IN | OUT)
    ids = np.arange(V, dtype=np.int32)

    def group_blob():
        top = e.group_topk_ranked(gid, 100, 0.0, gspec)
        pos, cnt = e.group_position_at(gid, ids[:500], gspec)
        smp = e.group_sample(gid, 64, gspec, seed=5)
        return b"".join([x.tobytes() for pair in top for x in pair] + [pos.tobytes(), cnt.tobytes()] + [np.asarray(x).tobytes() for x in smp])

    def track_blob():
        top = t.topk_ranked(100, 0.0, gspec)
        pos, cnt = t.position_at(ids[:500], gspec)
        smp = t.sample(64, gspec, seed=5)
        return b"".join([x.tobytes() for pair in top for x in pair] + [pos.tobytes(), cnt.tobytes(), t.rank_score_at(ids, gspec).tobytes()] +
                        [np.asarray(x).tobytes() for x in smp])

    g0 = group_blob()
    t0 = track_blob()
    assert group_blob() == g0 and track_blob() == t0 and group_blob() == g0   # the shared scratch and exclusion words serve both in turn
    held = eng.live_bytes()
    assert held[0] > base[0]
    for _ in range(3):   # the work space is the engine's and has its size: further calls allocate nothing
        track_blob()
    assert eng.live_bytes() == held
    t.close()
    e.close()
    assert eng.live_bytes() == base
