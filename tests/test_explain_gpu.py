"""Explain a score (dppr_explain_at / dppr_group_explain_at) against the numpy restatement of tests/explain_ref.py over what the
engine reports through its other calls: the dense columns from group_read / read, the out-CSR of the epoch by external id from
read_out_graph, the seeds of every lane. Integers are compared with array_equal, doubles by their bit patterns.

The order in which the device stores a row cannot be seen through read_out_graph (it returns every row sorted by EXTERNAL id), so
the assumption the kernels rest on -- the copies of a head are adjacent in the stored row, the row is sorted by internal id -- is
held to its consequences instead: `distinct` (which covers whole rows) and every `nbr_mult` (the up to 16 listed heads) equal
np.unique over (tail, head) at every vertex of the rig, under every step width of the hook (a run counted twice, or cut at a step
boundary, shows in either)."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import explain_ref as xr
from tests.test_explain_plan import unique_window
from tests.test_renumbering_gpu import churn_stream
from tests.test_targets_gpu import lane_kinds
from tests.test_weighted_gpu import EPS, Solved, star
from tests.util import small_stream

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 8, 10, 16)
SHAPES = ((16, 64), (3, 3), (1, 0), (0, 1))   # (f, depth)


def graph_of(e, epoch=-1):
    return xr.from_csr(*e.read_out_graph(epoch))


def cols_of(e, gid, n):
    return [e.group_read(gid, i)[0] for i in range(n)]


def check(e, gid, seeds, ids, f, depth, what, g=None, cols=None):
    """group_explain_at against the reference; returns (got, want)."""
    g = g if g is not None else graph_of(e)
    cols = cols if cols is not None else cols_of(e, gid, len(seeds))
    got = e.group_explain_at(gid, ids, f, depth)
    want = xr.explain(g, cols, seeds, ids, f, depth)
    assert got.keys() == want.keys()
    xr.same(got, want, what)
    return got, want


@pytest.fixture(scope="module", params=[1, 0], ids=["directed", "undirected"])
def solved(request):
    s = Solved(request.param, widths=WIDTHS)
    s.directed = request.param
    yield s
    s.e.close()


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_row_width(solved):
    s = solved
    e = s.e
    ids = np.arange(s.V, dtype=np.int32)
    assert s.V == 512
    seen_mult = seen_depth = seen_dead = seen_seed = 0
    for state in ("init", "two updates"):
        if state != "init":
            s.update(2)
        g = graph_of(e)
        for n, gid in s.groups.items():
            cols = cols_of(e, gid, n)
            for f, depth in SHAPES:
                _, want = check(e, gid, s.srcs[:n], ids, f, depth, (s.directed, state, n, f, depth), g, cols)
                seen_mult += int((want["nbr_mult"] > 1).sum())
                if depth == 3:
                    seen_depth += int((want["end"] == xr.END_DEPTH).sum())
                seen_dead += int((want["end"] == xr.END_DEAD).sum())
                seen_seed += int((want["end"] == xr.END_SEED).sum())
        # a run of equal heads across every step boundary: the widest group again, a wave taking 7 entries and 1 entry per step
        n, gid = 16, s.groups[16]
        cols = cols_of(e, gid, n)
        for rows in (7, 1):
            e.debug_explain(-1, rows)
            check(e, gid, s.srcs[:n], ids, 16, 64, (s.directed, state, "wave_rows", rows), g, cols)
        e.debug_explain(-1, 64)
    # the conditions on the rig
    assert seen_mult > 0 and seen_depth > 0 and seen_dead > 0 and seen_seed > 0, (seen_mult, seen_depth, seen_dead, seen_seed)
    assert np.any(g.mult > 1) and (s.directed or np.any(g.deg > 64))   # duplicate edges; undirected: a row longer than one step of a wave


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_slot_equals_a_one_lane_group():
    """Two solves of one source need not agree to the bit (the single-source solver pushes with float atomics, the group gathers;
    tests/test_changes_cli.py), so the slot is GIVEN the group's state: dppr_write puts the group's p and r into it, the read back
    is asserted equal bit for bit, and the slot form is then held to the one-lane group value for value -- and, as the write
    leaves the slot unconverged, without convergence."""
    V, e1, e2 = small_stream()
    e = eng.Engine(V, 600, 1, 20, schedule=eng.SCHEDULE_SYNC)
    e.load_window(e1[:600], e2[:600])
    src = int(datagen.top_sources(V, e1, e2, 600, 1, 1)[0])
    slot, gid = e.add_source(src), e.add_source_group([src])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    p_group, r_group = e.group_read(gid, 0)
    e.write(slot, p_group, r_group)
    p_slot, r_slot = e.read(slot)
    assert np.array_equal(p_slot.view(np.uint64), p_group.view(np.uint64)) and np.array_equal(r_slot.view(np.uint64), r_group.view(np.uint64))
    assert np.count_nonzero(p_group) > 100
    ids = np.arange(V, dtype=np.int32)
    g = graph_of(e)
    for f, depth in SHAPES:
        one = e.explain_at(slot, ids, f, depth)
        xr.same(one, xr.slot_form(xr.explain(g, [p_slot], [src], ids, f, depth)), ("slot", f, depth))
        grp, _ = check(e, gid, [src], ids, f, depth, ("one lane", f, depth), g, [p_group])
        xr.same(one, xr.slot_form(grp), ("slot against group", f, depth))
        assert one["self"].shape == (V,) and one["nbr"].shape == (V, f) and one["path"].shape == (V, depth + 1) and one["path_c"].shape == (V, depth)
    assert e.explain_at(slot, [src], 1, 1)["end"].tolist() == [xr.END_SEED] and e.explain_at(slot, [src], 1, 1)["self"].tolist() == [0.15]
    # defaults: f = 4, depth = 16
    d = e.explain_at(slot, ids[:5])
    assert d["nbr"].shape == (5, 4) and d["path"].shape == (5, 17)
    # want: only what is asked for is computed and returned
    few = e.group_explain_at(gid, ids, 3, 3, want=("len", "nbr_c"))
    full = e.group_explain_at(gid, ids, 3, 3)
    assert sorted(few) == ["len", "nbr_c"]
    xr.same(few, {k: full[k] for k in few}, "want")
    assert sorted(e.explain_at(slot, ids, 3, 3, want="deg")) == ["deg"]
    with pytest.raises(ValueError):
        e.explain_at(slot, ids, 3, 3, want=("len", "nope"))
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_set_lanes():
    """A target group of all five kinds of lane (tests/test_targets_gpu.py): self = 0.15 * weight, a path ends at ANY seed of a set."""
    V, W, c, batches = 4096, 1500, 100, 4
    e1, e2 = churn_stream(V, W + batches * c, 400, 6)
    kinds = lane_kinds(V, e1, np.random.default_rng(45))
    sets = [kinds[(i + 1) % 5] for i in range(5)]
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.load_window(*g.window_edges())
    gid = e.add_target_group(sets)
    e.group_init_solve(gid, EPS)
    for _ in range(batches):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.group_update(gid, EPS)
    seeds = [list(zip(ids.tolist(), w.tolist())) for ids, w in sets]
    rng = np.random.default_rng(3)
    ids = np.concatenate([np.concatenate([s[0] for s in sets]), rng.integers(0, V, 600)]).astype(np.int32)
    got, want = check(e, gid, seeds, ids, 4, 16, "set lanes")
    for i, (sid, w) in enumerate(sets):
        at = {int(v): j for j, v in enumerate(ids[:sum(len(s[0]) for s in sets)])}
        rows = [at[int(v)] for v in sid]
        assert np.array_equal(got["self"][rows, i], 0.15 * w) and np.all(got["end"][rows, i] == xr.END_SEED) and np.all(got["len"][rows, i] == 1)
    # a path that starts outside a set of several seeds and ends in it, at a seed that is not the set's first
    multi = [i for i, s in enumerate(sets) if len(s[0]) > 1]
    ends = [(i, int(got["path"][j, i, got["len"][j, i] - 1])) for i in multi for j in range(len(ids))
            if got["end"][j, i] == xr.END_SEED and got["len"][j, i] > 1]
    assert ends and any(v != int(np.sort(sets[i][0])[0]) for i, v in ends) and all(v in sets[i][0] for i, v in ends)
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def solved_on_device(V, tails, heads, source):
    e = eng.Engine(V, len(tails), 1, 1, schedule=eng.SCHEDULE_SYNC)
    e.load_window(np.asarray(tails, dtype=np.int32), np.asarray(heads, dtype=np.int32))
    gid = e.add_source_group([source])
    e.group_init_solve(gid, 1e-12)
    return e, gid


def every_way(e, gid, seeds, ids, f, depth, what):
    """The call under every step width and with the memo off and on: identical results, equal to the reference."""
    first = None
    for rows in (64, 7, 1):
        for memo in (0, 1):
            e.debug_explain(memo, rows)
            got, _ = check(e, gid, seeds, ids, f, depth, (what, rows, memo))
            first = first or got
            xr.same(got, first, (what, rows, memo, "against the first run"))
    e.debug_explain(-1, 64)
    return first


def test_hand_cases_on_the_device():
    # the three-vertex multigraph: both paths turn back at their second vertex
    tails, heads = [1] * 5 + [2] * 5 + [1, 2], [2] * 5 + [1] * 5 + [0, 0]
    e, gid = solved_on_device(64, tails, heads, 0)
    p = e.group_read(gid, 0)[0]
    assert abs(p[0] - 0.15) < 1e-9 and abs(p[1] - 0.1275 / 2.75) < 1e-9 and abs(p[2] - 0.1275 / 2.75) < 1e-9
    got = every_way(e, gid, [0], [0, 1, 2, 1, 3], 4, 8, "cycle")
    assert got["end"][:, 0].tolist() == [xr.END_SEED, xr.END_CYCLE, xr.END_CYCLE, xr.END_CYCLE, xr.END_DEAD]
    assert got["len"][:, 0].tolist() == [1, 2, 2, 2, 1] and got["path"][1, 0, :3].tolist() == [1, 2, -1]
    assert got["nbr"][1, 0].tolist() == [2, 0, -1, -1] and got["nbr_mult"][1, 0].tolist() == [5, 1, 0, 0]
    assert got["deg"].tolist() == [0, 6, 6, 6, 0] and got["distinct"].tolist() == [0, 2, 2, 2, 0]
    e.close()
    # the chain of 16
    e, gid = solved_on_device(64, np.arange(15, 0, -1), np.arange(14, -1, -1), 0)
    for depth, end, length in ((15, xr.END_SEED, 16), (64, xr.END_SEED, 16), (14, xr.END_DEPTH, 15)):
        got = every_way(e, gid, [0], [15, 7, 0], 2, depth, ("chain", depth))
        assert got["end"][0, 0] == end and got["len"][0, 0] == length
        assert got["path"][0, 0, :length].tolist() == list(range(15, 15 - length, -1))
        assert got["len"][1:, 0].tolist() == [8, 1] and got["end"][1:, 0].tolist() == [xr.END_SEED, xr.END_SEED]
    e.close()
    # a vertex whose best head is its own self loop
    e, gid = solved_on_device(64, [1, 1, 1, 1, 2], [1, 1, 1, 0, 1], 0)
    got = every_way(e, gid, [0], [1, 2, 3], 2, 5, "self loop")
    assert got["nbr"][0, 0].tolist() == [1, 0] and got["nbr_mult"][0, 0].tolist() == [3, 1]
    assert got["end"][:, 0].tolist() == [xr.END_CYCLE, xr.END_CYCLE, xr.END_DEAD] and got["len"][:, 0].tolist() == [1, 2, 1]
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_ties_are_cut_by_external_id():
    """The star of tests/test_weighted_gpu.py (both directions stored): the leaves enter in a shuffled order, so the hub's row is
    in internal order and the ties among its 1500 heads -- for a leaf lane all but one -- are cut by EXTERNAL id."""
    L = 1500
    e, gid, leaves, sources = star(L, lambda lv: [0, int(lv[5]), int(lv[17])])
    id_map = e.id_map()
    assert not np.all(np.diff(id_map[np.sort(leaves)]) > 0)   # internal order is not external order
    ids = np.concatenate([[0], leaves[:40], [int(sources[1]), 0, 4095 if 4095 not in leaves else 0]]).astype(np.int32)
    runs = []
    for rows in (64, 7, 1):
        for memo in (0, 1):
            e.debug_explain(memo, rows)
            runs.append(check(e, gid, sources, ids, 16, 64, ("star", rows, memo))[0])
    e.debug_explain(-1, 64)
    for other in runs[1:]:
        for k in runs[0]:
            assert runs[0][k].tobytes() == other[k].tobytes(), k
    got = runs[0]
    assert got["deg"][0] == L and got["distinct"][0] == L
    hub = got["nbr"][0, 1]                    # the hub's contributors in the lane of leaf 5: that leaf, then the tie in id order
    rest = np.sort(leaves[leaves != sources[1]])
    assert hub[0] == sources[1] and np.array_equal(hub[1:], rest[:15])
    assert len(np.unique(got["nbr_c"][0, 1, 1:])) == 1
    for bad in ((-2, 64), (2, 64), (0, 0), (0, 65), (1, -1)):
        with pytest.raises(eng.DpprError):
            e.debug_explain(*bad)
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_id_space_parked_and_unnamed_vertices():
    """The churn rig of tests/test_rank_gpu.py after renumberings: parked and unnamed ids have no row in the epoch, paths name
    external ids."""
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
    n_parked = sp["parked"]
    assert n_parked > 0 and sp["renumberings"] > 0, sp
    id_map = e.id_map()
    unnamed = np.nonzero(id_map < 0)[0]
    parked = np.nonzero(id_map >= V - n_parked)[0]
    live = np.nonzero((id_map >= 0) & (id_map < sp["ids"]))[0]
    assert len(unnamed) > 0 and len(parked) == n_parked
    assert not np.array_equal(id_map[live], live)   # the numbering is not the identity: an internal id in a path would show
    ids = np.concatenate([parked[:200], unnamed[:200], live[::3]]).astype(np.int32)
    assert len(ids) <= eng.EXPLAIN_MAX_M
    got, _ = check(e, gid, [0, 1, 2], ids, 4, 16, "churn")
    gone = np.isin(ids, np.concatenate([parked, unnamed]))
    assert np.all(got["deg"][gone] == 0) and np.all(got["distinct"][gone] == 0)
    seeds = np.array([0, 1, 2])
    for i in range(3):
        not_seed = gone & (ids != seeds[i])
        assert np.all(got["len"][not_seed, i] == 1) and np.all(got["end"][not_seed, i] == xr.END_DEAD) and np.all(got["nbr_count"][not_seed, i] == 0)
    cols = cols_of(e, gid, 3)
    pk = np.isin(ids, parked)
    assert any(np.any(got["path_p"][pk, i, 0] > 0) for i in range(3))            # a parked vertex keeps its p
    assert all(np.array_equal(got["path_p"][:, i, 0].view(np.uint64), cols[i][ids].view(np.uint64)) for i in range(3))
    assert np.any(got["len"] > 2)
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_prefix_and_monotone_properties(directed):
    W, c = 600, 20
    V, e1, e2 = unique_window(directed, W)
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 5)]
    g = orc.Graph(V, e1, e2, directed, W, c)
    e = eng.Engine(V, W, directed, c)
    e.load_window(*g.window_edges())
    gid = e.add_source_group(srcs)
    e.group_init_solve(gid, 1e-9)
    ids = np.arange(V, dtype=np.int32)
    graph = graph_of(e)
    assert np.all(graph.mult == 1) and np.all(graph.tail != graph.head)   # a simple graph
    full, _ = check(e, gid, srcs, ids, 1, 64, ("simple", directed), graph)
    # the prefix property over depth
    for depth in (0, 1, 2, 3):
        cut = e.group_explain_at(gid, ids, 1, depth)
        n_full = full["len"]
        assert np.array_equal(cut["len"], np.minimum(n_full, depth + 1))
        # a path that ended before the cut keeps its end; one that ends AT the cut keeps a seed (rule 1 comes before rule 2) and is
        # otherwise cut there; a longer one is cut
        at_cut_seed = (n_full == depth + 1) & (full["end"] == xr.END_SEED)
        assert np.array_equal(cut["end"], np.where(n_full < depth + 1, full["end"], np.where(at_cut_seed, xr.END_SEED, xr.END_DEPTH)))
        assert np.any(n_full > depth + 1)
        assert np.array_equal(cut["path"], full["path"][:, :, :depth + 1])
        assert np.array_equal(cut["path_p"].view(np.uint64), full["path_p"][:, :, :depth + 1].view(np.uint64))
        assert np.array_equal(cut["path_c"].view(np.uint64), np.ascontiguousarray(full["path_c"][:, :, :depth]).view(np.uint64))
    # the monotone property: on a simple graph the arg-max of c is the arg-max of p, and the invariant gives max_w p[w] > 1.17 p[u]
    bound = math.ceil(math.log(1e4) / math.log(1.176)) + 1
    cols = cols_of(e, gid, 5)
    for i in range(5):
        starts = np.nonzero(cols[i] > 1e-4)[0]
        assert len(starts) > 50
        for u in starts:
            n = int(full["len"][u, i])
            assert full["end"][u, i] == xr.END_SEED and n <= bound and full["path"][u, i, n - 1] == srcs[i], (i, u)
            assert np.all(np.diff(full["path_p"][u, i, :n]) > 0), (i, u)
    e.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_on_a_live_engine():
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
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    M, F, D = 8, 3, 4
    ints, dbls = np.full(2 * M * (D + 1) * 4, 77, dtype=np.int32), np.full(2 * M * (D + 1) * 4, 7.5)
    out = eng.ExplainOut()
    for name, _ in eng.ExplainOut._fields_:
        setattr(out, name, (dbls.ctypes.data_as(dp) if name in ("self", "nbr_c", "path_p", "path_c") else ints.ctypes.data_as(ip)))
    at = np.arange(M, dtype=np.int32)
    A, O = at.ctypes.data_as(ip), C.byref(out)

    def refused(epoch=-1, ids=A, m=M, f=F, depth=D, o=O, group=gid, slot_=slot):
        rcs = (L.dppr_group_explain_at(h, group, epoch, ids, m, f, depth, o), L.dppr_explain_at(h, slot_, epoch, ids, m, f, depth, o))
        return rcs == (-1, -1) and bool(np.all(ints == 77) and np.all(dbls == 7.5))

    big = np.zeros(eng.EXPLAIN_MAX_M + 1, dtype=np.int32)
    for kw in (dict(m=-1), dict(ids=big.ctypes.data_as(ip), m=eng.EXPLAIN_MAX_M + 1), dict(ids=None), dict(o=None), dict(f=-1), dict(f=17),
               dict(depth=-1), dict(depth=65), dict(f=0, depth=0), dict(ids=np.array([0, -1] * 4, dtype=np.int32).ctypes.data_as(ip)),
               dict(ids=np.array([V, 0] * 4, dtype=np.int32).ctypes.data_as(ip)), dict(group=5, slot_=5), dict(group=-1, slot_=-1)):
        assert refused(**kw), list(kw)
    # the epoch rule of dppr_cluster
    e.read_out_graph(newest - 1)  # (resident)
    assert refused(newest - 1) and b"another epoch" in L.dppr_last_error(h)
    assert refused(newest - 2) and refused(newest + 1) and b"not resident" in L.dppr_last_error(h)
    # m == 0 is valid and writes nothing, with or without pointers; so is a call that asks for nothing
    assert L.dppr_group_explain_at(h, gid, -1, None, 0, F, D, None) == 0 and L.dppr_group_explain_at(h, gid, -1, A, 0, F, D, O) == 0
    assert L.dppr_group_explain_at(h, gid, -1, A, M, F, D, C.byref(eng.ExplainOut())) == 0
    assert np.all(ints == 77) and np.all(dbls == 7.5)
    assert e.group_explain_at(gid, np.zeros(0, dtype=np.int32), F, D)["path"].shape == (0, 2, D + 1)
    # the limits themselves are accepted, only what is asked for is written, and exactly the documented shape
    res = e.group_explain_at(gid, big[:eng.EXPLAIN_MAX_M], 16, 64)
    assert res["path"].shape == (eng.EXPLAIN_MAX_M, 2, 65) and np.all(res["path"][:, :, 0] == 0)
    only = eng.ExplainOut()
    lens = np.full(2 * M + 3, 77, dtype=np.int32)
    only.len = lens.ctypes.data_as(ip)
    assert L.dppr_group_explain_at(h, gid, newest, A, M, F, D, C.byref(only)) == 0
    want = xr.explain(graph_of(e), cols_of(e, gid, 2), srcs, at, F, D)
    assert np.array_equal(lens[:2 * M].reshape(M, 2), want["len"]) and np.all(lens[2 * M:] == 77)
    e.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_after_another_family_and_every_buffer_goes_with_the_engine():
    """group_topk_ranked runs first on one engine, so the scratch state the memo lies in is already there; on it as on a fresh engine
    the result is the reference's over that engine's own state (two eager solves do not agree to the bit), the device time is
    reported, and all of it goes with the engine."""
    gc.collect()
    before = eng.live_bytes()
    for warm in (True, False):
        s = Solved(1, widths=(10,))
        gid = s.groups[10]
        s.update(1)
        if warm:
            s.e.group_topk_ranked(gid, 100, 0.0, None)
        held = eng.live_bytes()
        s.e.set_profiling(1)
        s.e.debug_explain(1, 64)
        got, _ = check(s.e, gid, s.srcs[:10], np.arange(s.V, dtype=np.int32), 16, 64, ("warm", warm))
        assert got["nbr_count"].max() > 1 and got["len"].max() > 2
        assert eng.live_bytes()[0] > held[0] and eng.live_bytes()[1] > held[1]   # (the block and its pinned twin are there)
        assert s.e.query_ms() > 0.0
        s.e.close()
    assert eng.live_bytes() == before
