"""Weighted vertex sets as the targets of a group (dppr_add_target_group / dppr_group_replace_target / dppr_group_targets) on the
device, against tests/targets_ref.py: the fixed point of the invariant with h, and the invariant itself.

The bounds, per lane (every lane here is normalised to sum(h) <= 1, so p <= 1):
    |p - exact_p| < eps + 1e-13     (|e|_inf <= |r|_inf < eps for any h, include/dppr.h; 1e-13: the project's rounding allowance)
    max|r| < eps
    invariant_err < 1e-13           (the bound of tests/test_renumbering_gpu.py and tests/test_oracle_golden.py)"""
import os
import subprocess

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests import cluster_ref, targets_ref
from tests.cf_stream import conflict_free_stream
from tests.test_conflict_free_streams import EPS as CF_EPS, SMALL
from tests.test_renumbering_gpu import churn_stream
from tests.util import window_directed_edges

pytestmark = pytest.mark.gpu

EPS = 1e-9
ROUND = 1e-13
INV_TOL = 1e-13


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def advance(g, e):
    assert not g.stream_updates()
    g.inc_construct(1)
    e.set_batch(*g.batch())
    e.slide(*g.new_stream())


def h_matrix(sets, V):
    return np.stack([targets_ref.seed_vector(i, w, V) for i, w in sets], axis=1)


def check_lanes(e, gid, sets, g, V, eps, tag, exact=True):
    """The three bounds for every lane of the group; the figures are printed before they are asserted."""
    src, dst = window_directed_edges(g)
    H = h_matrix(sets, V)
    want = targets_ref.exact_p(H, src, dst, V) if exact else None
    for i in range(len(sets)):
        p, r = e.group_read(gid, i)
        rmax = float(np.max(np.abs(r)))
        inv = targets_ref.invariant_err(p, r, H[:, i], src, dst, V)
        gap = float(np.max(np.abs(p - want[:, i]))) if exact else 0.0
        print("lane", tag, i, len(sets[i][0]), "max|r|", rmax, "invariant", inv, "|p - exact|", gap)
        assert rmax < eps, (tag, i, rmax)
        assert inv < INV_TOL, (tag, i, inv)
        assert gap < eps + ROUND, (tag, i, gap)


def other(v, avoid):
    """v, or the next vertex that is not in `avoid` (a lane holds no vertex twice)."""
    v = int(v)
    while v in avoid:
        v += 1
    return v


def lane_kinds(V, e1, rng):
    """The five kinds of lane of case 1, each normalised to sum(h) <= 1."""
    w300 = rng.random(300) + 0.01
    band = np.unique(np.concatenate([[int(e1[0])], rng.choice(V, 6, replace=False)]))
    return [
        (np.array([1], dtype=np.int32), np.array([1.0])),                                         # a single seed of weight 1.0
        (np.array([2, other(e1[7], (2,))], dtype=np.int32), np.array([0.7, 0.2])),                        # 2 seeds, unequal weights
        (rng.choice(V, 40, replace=False).astype(np.int32), np.full(40, 1.0 / 40)),               # 40 uniform seeds
        (rng.choice(V, 300, replace=False).astype(np.int32), w300 / w300.sum()),                  # 300 random weights, normalised
        (band.astype(np.int32), np.full(len(band), 0.125)),                                       # holds e1[0], the band vertex that retires early
    ]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 8, 10, 16])
@pytest.mark.parametrize("directed", [1, 0])
def test_values_every_row_width(directed, n):
    V, W, c, batches = 4096, 1500, 100, 20
    e1, e2 = churn_stream(V, W + batches * c, 400, 5 + directed)
    rng = np.random.default_rng(40 + n)
    kinds = lane_kinds(V, e1, rng)
    assert int(e1[0]) in kinds[4][0]
    sets = [kinds[(i + 1) % 5] for i in range(n)]  # (n = 1: the two-seed set; from n = 5 on every kind)
    g = orc.Graph(V, e1, e2, directed, W, c)
    e = eng.Engine(V, W, directed, c)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    gid = e.add_target_group(sets)
    e.group_init_solve(gid, EPS)
    check_lanes(e, gid, sets, g, V, EPS, ("init", directed, n))
    for k in range(1, batches + 1):
        advance(g, e)
        e.group_update(gid, EPS)
        check_lanes(e, gid, sets, g, V, EPS, (k, directed, n))
    sp, m = e.id_space(), e.id_map()
    print("id space", sp)
    assert sp["renumberings"] >= 3 and sp["parked"] > 0, sp
    seeds = np.unique(np.concatenate([i for i, _ in sets]))
    assert np.all(m[seeds] >= 0) and np.all(m[seeds] < sp["ids"]), "a seed is parked"
    if n >= 5:  # 6 queries ride along: top-k is the sort of the dense read, the cluster of a set lane is the reference's
        topk = e.group_topk(gid, 50)
        row, col = e.read_out_graph()
        for i in range(n):
            p, _ = e.group_read(gid, i)
            order = np.lexsort((np.arange(V), -p))[:50]
            order = order[p[order] > 0.0]
            assert np.array_equal(topk[i][0], order) and np.array_equal(bits(topk[i][1]), bits(p[order])), i
        lane = next(i for i, s in enumerate(sets) if len(s[0]) == 300)
        best, ids, co, ci, vol = e.group_cluster(gid, 50, profile=True)
        want = cluster_ref.cluster(V, row, col, len(col), topk[lane][0], 50, 1)
        assert best[lane]["count"] == want[0]["count"] and best[lane]["best_size"] == want[0]["best_size"]
        assert best[lane]["best_cut"] == want[0]["best_cut"] and best[lane]["best_vol"] == want[0]["best_vol"]
        assert bits(np.array([best[lane]["best_phi"]]))[0] == bits(np.array([want[0]["best_phi"]]))[0]
        assert np.array_equal(ids[lane], want[1]) and np.array_equal(co[lane], want[2]) and np.array_equal(ci[lane], want[3])
        assert np.array_equal(vol[lane], want[4])
    e.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_single_seeds_of_weight_one_are_a_source_group():
    """A target group of single seeds of weight 1.0 against add_source_group on a second engine: the same sources, r bit-equal
    right after creation, p and r bit-equal after the solve and 10 batches of a conflict-free stream (two plain engines give equal
    bits there; on R-MAT streams they differ in the last bits already)."""
    shape = dict(SMALL, batches=10)
    V, e1, e2, meta = conflict_free_stream(seed=2, **shape)
    W, c = shape["W"], shape["c"]
    sources = [int(x) for x in meta["sources"][:5]]
    engines = []
    for targets in (True, False):
        g = orc.Graph(V, e1, e2, 1, W, c)
        e = eng.Engine(V, W, 1, c)
        e.load_window(*g.window_edges())
        gid = e.add_target_group([([s], [1.0]) for s in sources]) if targets else e.add_source_group(sources)
        engines.append((g, e, gid))
    (_, a, ga), (_, b, gb) = engines
    assert a.group_sources(ga) == b.group_sources(gb) == sources
    assert [(i.tolist(), w.tolist()) for i, w in a.group_targets(ga)] == [([s], [1.0]) for s in sources]
    assert [(i.tolist(), w.tolist()) for i, w in b.group_targets(gb)] == [([s], [1.0]) for s in sources]

    def same_state(tag):
        for i in range(len(sources)):
            (pa, ra), (pb, rb) = a.group_read(ga, i), b.group_read(gb, i)
            assert np.array_equal(bits(pa), bits(pb)) and np.array_equal(bits(ra), bits(rb)), (tag, i)

    same_state("created")
    assert a.group_read(ga, 1)[1][sources[1]] == 1.0
    for _, e, gid in engines:
        e.group_init_solve(gid, CF_EPS)
    same_state("solved")
    for k in range(10):
        for g, e, gid in engines:
            advance(g, e)
            e.group_update(gid, CF_EPS)
        same_state(k)
    assert a.group_stats(ga)["sum_E"] == b.group_stats(gb)["sum_E"]
    a.close()
    b.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def long_run_stream(V, W, c, u, rng):
    """Directed stream, W / c = 4: the seed vertex u is the tail of 200 inserts of batch 1 (no delete), of 100 deletes and 100
    inserts of batch 2, of 50 inserts of batch 3 and of 25 deletes and 25 inserts of batch 4 -- runs of 200 records (the wave
    path, beyond SU_LONG = 96) and of 50 (the per-lane path). u's heads are all different; nothing else has u as its tail."""
    n = W + 4 * c
    e1 = rng.integers(1, V, n).astype(np.int64)
    e1[e1 == u] = u + 1
    e2 = rng.integers(0, V, n).astype(np.int64)
    heads = rng.permutation(np.setdiff1d(np.arange(V), [u]))
    at = 0
    for lo, cnt in ((c, 100), (3 * c, 25), (W, 200), (W + c, 100), (W + 2 * c, 50), (W + 3 * c, 25)):
        pos = lo + rng.choice(c, cnt, replace=False)
        e1[pos] = u
        e2[pos] = heads[at:at + cnt]
        at += cnt
    same = e1 == e2
    e2[same] = (e2[same] + 1) % V
    assert not np.any((e1 == u) & (e2 == u))
    return e1.astype(np.int32), e2.astype(np.int32)


def test_long_tail_runs_take_both_paths_of_the_seeded_update():
    """A missing ALPHA * h[u] in either path of k_su_apply_seeded leaves an invariant error of order h / (d + 1) at u."""
    V, W, c, u = 2048, 1024, 256, 700
    rng = np.random.default_rng(9)
    e1, e2 = long_run_stream(V, W, c, u, rng)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.load_window(*g.window_edges())
    sets = [(np.array([u, 5], dtype=np.int32), np.array([0.6, 0.4])),
            (np.array([3, 9], dtype=np.int32), np.array([0.5, 0.5])),   # u is no seed here: h[u] = 0
            (np.array([u], dtype=np.int32), np.array([1.0])),            # a source lane in a group that has set lanes
            (np.array([u], dtype=np.int32), np.array([0.25]))]
    gid = e.add_target_group(sets)
    assert e.group_sources(gid) == [-1, -1, u, -1]
    e.group_init_solve(gid, EPS)
    for k, (run, dels) in enumerate(((200, 0), (200, 100), (50, 0), (50, 25)), start=1):
        advance(g, e)
        b1, _, ins = g.batch()
        mine = b1 == u
        assert mine.sum() == run and (ins[mine] == 0).sum() == dels, (k, mine.sum())
        e.group_update(gid, EPS)
        check_lanes(e, gid, sets, g, V, EPS, ("run", run, dels))
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_churn_of_a_group_with_set_lanes():
    V, W, c, directed = 4096, 1500, 100, 0
    e1, e2 = churn_stream(V, W + 8 * c, 400, 17)
    rng = np.random.default_rng(4)
    g = orc.Graph(V, e1, e2, directed, W, c)
    e = eng.Engine(V, W, directed, c)
    e.load_window(*g.window_edges())
    src = lambda v: (np.array([v], dtype=np.int32), np.array([1.0]))
    w40 = rng.random(40) + 0.1
    set1 = (np.sort(rng.choice(V, 40, replace=False)).astype(np.int32), w40 / w40.sum())
    set3 = (np.array([2, 3, other(e1[3], (2, 3))], dtype=np.int32), np.array([0.5, 0.25, 0.125]))
    sets = [src(0), set1, src(1), set3, src(int(e1[0]))]
    gid = e.add_target_group(sets)
    assert e.group_sources(gid) == [0, -1, 1, -1, int(e1[0])]
    e.group_init_solve(gid, EPS)
    advance(g, e)
    e.group_update(gid, EPS)
    check_lanes(e, gid, sets, g, V, EPS, "before")

    # replace_target of lane 1: the other lanes bit-equal, the new lane within eps of exact_p; the mark is dropped
    e.group_mark(gid)
    e.group_changes(gid, 4)
    before = [e.group_read(gid, i) for i in range(5)]
    w7 = rng.random(7) + 0.1
    new1 = (np.sort(rng.choice(V, 7, replace=False)).astype(np.int32), w7 / w7.sum() * 0.9)
    assert e.group_replace_target(gid, 1, new1[0][::-1], new1[1][::-1]) >= 0.0
    sets[1] = new1
    with pytest.raises(eng.DpprError):
        e.group_changes(gid, 4)
    for i in (0, 2, 3, 4):
        p, r = e.group_read(gid, i)
        assert np.array_equal(bits(p), bits(before[i][0])) and np.array_equal(bits(r), bits(before[i][1])), i
    check_lanes(e, gid, sets, g, V, EPS, "replace_target")
    got = e.group_targets(gid)
    assert np.array_equal(got[1][0], new1[0]) and np.array_equal(bits(got[1][1]), bits(new1[1]))

    # remove_source(0): the sets move down with their lanes; the next update keeps the invariant
    e.group_remove_source(gid, 0)
    del sets[0]
    assert e.group_sources(gid) == [-1, 1, -1, int(e1[0])]
    got = e.group_targets(gid)
    assert len(got) == 4
    for (gi, gw), (wi, ww) in zip(got, sets):
        assert np.array_equal(gi, np.sort(wi)) and np.array_equal(bits(gw), bits(ww[np.argsort(wi)]))
    advance(g, e)
    e.group_update(gid, EPS)
    check_lanes(e, gid, sets, g, V, EPS, "remove_source")

    # add_source, then a batch
    idx, _ = e.group_add_source(gid, 7)
    assert idx == 4
    sets.append(src(7))
    assert e.group_sources(gid) == [-1, 1, -1, int(e1[0]), 7]
    check_lanes(e, gid, sets, g, V, EPS, "add_source")
    advance(g, e)
    e.group_update(gid, EPS)
    check_lanes(e, gid, sets, g, V, EPS, "add_source + batch")

    # replace_source on a set lane: a source lane
    e.group_mark(gid)
    e.group_replace_source(gid, 0, 11)
    sets[0] = src(11)
    assert e.group_sources(gid) == [11, 1, -1, int(e1[0]), 7]
    with pytest.raises(eng.DpprError):
        e.group_changes(gid, 4)
    check_lanes(e, gid, sets, g, V, EPS, "replace_source")
    # ... and the last set lane: the group is a source group again, and goes on as one
    e.group_replace_source(gid, 2, 12)
    sets[2] = src(12)
    assert e.group_sources(gid) == [11, 1, 12, int(e1[0]), 7]
    assert [(i.tolist(), w.tolist()) for i, w in e.group_targets(gid)] == [([s], [1.0]) for s in (11, 1, 12, int(e1[0]), 7)]
    advance(g, e)
    e.group_update(gid, EPS)
    check_lanes(e, gid, sets, g, V, EPS, "sources again")
    # ... and the first set lane of a source group
    e.group_replace_target(gid, 4, set3[0], set3[1])
    sets[4] = set3
    assert e.group_sources(gid) == [11, 1, 12, int(e1[0]), -1]
    advance(g, e)
    e.group_update(gid, EPS)
    check_lanes(e, gid, sets, g, V, EPS, "a set lane again")
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_listing_and_rejections():
    V, W, c = 512, 600, 20
    rng = np.random.default_rng(6)
    e1, e2 = rng.integers(0, 300, W + 2 * c).astype(np.int32), rng.integers(0, 300, W + 2 * c).astype(np.int32)
    e2[e1 == e2] = (e2[e1 == e2] + 1) % 300
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.load_window(*g.window_edges())
    given = [([9], [1.0]), ([30, 10, 20], [0.3, 0.1, 0.2]), ([9, 2], [0.5, 0.25]), ([500], [0.5])]  # (500: no edge in the window)
    gid = e.add_target_group(given)
    got = e.group_targets(gid)
    assert [(i.tolist(), w.tolist()) for i, w in got] == [([9], [1.0]), ([10, 20, 30], [0.1, 0.2, 0.3]), ([2, 9], [0.25, 0.5]), ([500], [0.5])]
    assert e.group_sources(gid) == [9, -1, -1, -1]
    assert e.id_map()[500] >= 0
    # the two-call protocol: the offsets are always true, a short cap leaves the arrays alone
    off, ids, w = e.group_targets(gid, cap=0)
    assert off.tolist() == [0, 1, 4, 6] + [7] * 13
    off, ids, w = e.group_targets(gid, cap=6)
    assert off[16] == 7 and np.all(ids == -7) and np.all(w == -7.0)
    off, ids, w = e.group_targets(gid, cap=7)
    assert ids.tolist() == [9, 10, 20, 30, 2, 9, 500] and w.tolist() == [1.0, 0.1, 0.2, 0.3, 0.25, 0.5, 0.5]
    L, h = e._L, e._h
    import ctypes as C
    i64p, ip, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    o17 = np.zeros(17, dtype=np.int64)
    assert L.dppr_group_targets(h, gid, None, None, None, 0) == -1 and L.dppr_group_targets(h, gid, o17.ctypes.data_as(i64p), None, None, -1) == -1
    assert L.dppr_group_targets(h, gid, o17.ctypes.data_as(i64p), None, None, 7) == -1 and L.dppr_group_targets(h, gid + 1, o17.ctypes.data_as(i64p), None, None, 0) == -1

    e.group_init_solve(gid, EPS)
    space, listed = e.id_space(), e.group_targets(gid, cap=7)

    def untouched():
        now = e.group_targets(gid, cap=7)
        return e.id_space() == space and all(np.array_equal(a, b) for a, b in zip(now, listed))

    def add(off, ids, w, n):
        off, ids, w = np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int32), np.asarray(w, dtype=np.float64)
        out = C.c_int32(-5)
        rc = L.dppr_add_target_group(h, off.ctypes.data_as(i64p), ids.ctypes.data_as(ip), w.ctypes.data_as(dp), n, C.byref(out))
        assert out.value == -5
        return rc

    def replace(index, ids, w, m=None, group=gid):
        ids, w = np.asarray(ids, dtype=np.int32), np.asarray(w, dtype=np.float64)
        return L.dppr_group_replace_target(h, group, index, ids.ctypes.data_as(ip), w.ctypes.data_as(dp), len(ids) if m is None else m, None)

    fresh = 400  # (a vertex without an id: a rejected call must not give it one)
    assert e.id_map()[fresh] < 0
    big = np.arange(eng.TARGET_SET_MAX + 1) % V
    cases = [
        add([0, 1], [fresh], [1.0], 0), add(np.zeros(18), [fresh] * 17, [1.0] * 17, 17),                       # n
        add([1, 2], [fresh, 1], [1.0, 1.0], 1), add([0, 2, 1], [fresh, 1], [1.0, 1.0], 2),                      # offsets
        add([0, 0, 1], [fresh], [1.0], 2), add([0, len(big)], big, np.ones(len(big)), 1),                       # lane sizes
        add([0, 2], [fresh, V], [1.0, 1.0], 1), add([0, 2], [fresh, -1], [1.0, 1.0], 1),                        # ids in [0, V)
        add([0, 3], [fresh, 5, fresh], [1.0, 1.0, 1.0], 1),                                                     # an id twice in a lane
        add([0, 2], [fresh, 5], [1.0, 0.0], 1), add([0, 2], [fresh, 5], [1.0, -0.5], 1),                        # weights
        add([0, 2], [fresh, 5], [1.0, np.nan], 1), add([0, 2], [fresh, 5], [np.inf, 1.0], 1),
        replace(1, [fresh, fresh], [0.5, 0.5]), replace(1, [fresh], [0.0]), replace(1, [V], [1.0]), replace(1, [fresh], [1.0], m=0),
        replace(4, [fresh], [0.5]), replace(-1, [fresh], [0.5]), replace(0, [fresh], [0.5], group=gid + 1),
    ]
    assert cases == [-1] * len(cases), cases
    assert untouched() and e.id_map()[fresh] < 0
    e.close()


def test_the_same_id_in_two_lanes_and_a_group_that_is_not_converged():
    V, W, c = 512, 600, 20
    rng = np.random.default_rng(8)
    e1, e2 = rng.integers(0, 300, W + 2 * c).astype(np.int32), rng.integers(0, 300, W + 2 * c).astype(np.int32)
    e2[e1 == e2] = (e2[e1 == e2] + 1) % 300
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.load_window(*g.window_edges())
    sets = [(np.array([4, 6], dtype=np.int32), np.array([0.5, 0.5])), (np.array([4], dtype=np.int32), np.array([0.75]))]
    gid = e.add_target_group(sets)
    with pytest.raises(eng.DpprError):  # (the contract of group_replace_source: converged first)
        e.group_replace_target(gid, 0, [1, 2], [0.5, 0.5])
    assert [(i.tolist(), w.tolist()) for i, w in e.group_targets(gid)] == [([4, 6], [0.5, 0.5]), ([4], [0.75])]
    e.group_init_solve(gid, EPS)
    check_lanes(e, gid, sets, g, V, EPS, "two lanes, one vertex")
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_cli_target_sets(tmp_path, directed):
    """./pagerank --target-sets on a toy .bin: --validate runs the set-lane check after the solve and after every batch and exits 0,
    and the dumped lanes satisfy the bounds of case 1 on the oracle's final window."""
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, read_dump, run
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    W, c, batches = 600, 6, 5
    top = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 12)]
    sets = [(np.array([top[0]], dtype=np.int32), np.array([1.0])),                       # a bare id: weight 1.0, a source lane
            (np.array(top[1:4], dtype=np.int32), np.array([0.5, 0.25, 0.125])),
            (np.array(top[4:12] + [V - 1], dtype=np.int32), np.full(9, 0.1))]
    lines = [str(top[0]), " ".join(f"{int(i)}:{float(w)!r}" for i, w in zip(*sets[1])), " ".join(f"{i}:0.1" for i in sets[2][0])]
    sf = tmp_path / "sets.txt"
    sf.write_text("\n".join(lines) + "\n")
    dump = str(tmp_path / "out.dump")
    r = run([BIN, "-d", path, "-a", "0", "-i", str(directed), "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", str(batches),
             "--target-sets", str(sf), "--validate", "--dump", dump, "--topk", "3"])
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("validate ok (set lane of") == 3 * (batches + 1), r.stdout
    assert "residual bound + invariant with h" in r.stdout and len([l for l in r.stdout.splitlines() if l.startswith("topk ")]) == 9
    g = orc.Graph(V, e1, e2, directed, W, c)
    for _ in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
    src, dst = window_directed_edges(g)
    lanes = read_dump(dump)
    assert sorted(lanes) == sorted(int(i[0]) for i, _ in sets)   # (a lane is named by its first id)
    want = targets_ref.exact_p(h_matrix(sets, V), src, dst, V)
    for k, (ids, w) in enumerate(sets):
        p, rr = lanes[int(ids[0])]
        h = targets_ref.seed_vector(ids, w, V)
        rmax, inv, gap = float(np.max(np.abs(rr))), targets_ref.invariant_err(p, rr, h, src, dst, V), float(np.max(np.abs(p - want[:, k])))
        print("cli lane", directed, k, "max|r|", rmax, "invariant", inv, "|p - exact|", gap)
        assert rmax < EPS and inv < INV_TOL and gap < EPS + ROUND
