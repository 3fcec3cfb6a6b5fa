"""The certificate of a state (dppr_certify / dppr_group_certify) against the numpy restatement of tests/certify_ref.py over what
the engine reports through its other calls: the dense columns from group_read / read, the stored out-edges of the epoch by external
id from read_out_graph, the id map, the seeds of every lane. Integers are compared with array_equal; max_abs_r, sum_abs_r and
sum_p by their bit patterns; inv_max_err to INVARIANT_TOL = 1e-13, the project's bound of the invariant (the device adds the heads
of a row in its own order), and identical bits between two calls with the same dppr_debug_certify setting."""
import ctypes as C
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import certify_ref as cr
from tests.test_dot_gpu import put
from tests.test_export_gpu import Hip
from tests.test_renumbering_gpu import churn_stream
from tests.test_targets_gpu import lane_kinds
from tests.test_weighted_gpu import EPS, Solved
from tests.util import small_stream

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 8, 10, 16)
INVARIANT_TOL = 1e-13
SETTINGS = ((0, 0), (7, 1), (64, 4), (0, 0))   # dppr_debug_certify(piece_edges, wave_rows)
RESIDUAL = ("max_abs_r", "argmax_r", "sum_abs_r", "sum_p", "n_pos", "n_neg", "n_nonfinite", "n_p_nonzero")
EXACT = RESIDUAL + ("state_epoch", "converged", "conv_eps")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def edges_of(e, epoch=-1):
    """The stored out-edges of an epoch by external id: (tails, heads), duplicates and self loops as stored."""
    row, col = e.read_out_graph(epoch)
    return np.repeat(np.arange(len(row) - 1), np.diff(row)), col.astype(np.int64)


def group_cols(e, gid, n):
    reads = [e.group_read(gid, i) for i in range(n)]
    return [p for p, _ in reads], [r for _, r in reads]


def same_residual(got, want, what):
    for k in RESIDUAL:
        if got[k].dtype == np.float64:
            assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, got[k], want[k])
        else:
            assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k, a[k], b[k])


def check(e, gid, seeds, eps, what, tails, heads, tol=None, epoch=-1):
    """group_certify against the reference over the dense reads; returns (got, want). tol [n]: the bound of every lane's invariant."""
    n = len(seeds)
    ps, rs = group_cols(e, gid, n)
    want = cr.certify(e.V, tails, heads, ps, rs, seeds, eps, has_id=e.id_map() >= 0)
    got = e.group_certify(gid, eps, epoch)
    same_residual(got, want, what)
    tol = np.full(n, INVARIANT_TOL) if tol is None else tol
    diff = np.abs(got["inv_max_err"] - want["inv_max_err"])
    print(what, "inv_max_err", got["inv_max_err"].max(), "reference", want["inv_max_err"].max(), "apart", diff.max())
    assert np.all(diff < tol), (what, got["inv_max_err"], want["inv_max_err"])
    return got, want


@pytest.fixture(scope="module", params=[1, 0], ids=["directed", "undirected"])
def solved(request):
    s = Solved(request.param, widths=WIDTHS)
    s.directed = request.param
    yield s
    s.e.close()


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_healthy_states_every_row_width(solved):
    s, e = solved, solved.e
    assert s.V == 512
    hip = Hip()
    d_ones = put(hip, np.ones((1, s.V)))
    first = e.group_certify(s.groups[1], EPS, invariant=False)["state_epoch"]   # the epoch of the loaded window
    epochs = {"init": first, "two updates": first + 2}
    assert first >= 0
    for state in ("init", "two updates"):
        if state != "init":
            s.update(2)
        tails, heads = edges_of(e)
        deg = np.bincount(tails, minlength=s.V)
        for n, gid in s.groups.items():
            runs = []
            for piece, wave_rows in SETTINGS:
                e.debug_certify(piece, wave_rows)
                what = (s.directed, state, n, piece, wave_rows)
                got, want = check(e, gid, s.srcs[:n], EPS, what, tails, heads)
                same_bits(got, e.group_certify(gid, EPS), what)           # a second call: identical bits in every output
                assert np.all(got["inv_max_err"] < INVARIANT_TOL), (what, got["inv_max_err"])
                assert np.all(got["n_pos"] == 0) and np.all(got["n_neg"] == 0) and np.all(got["n_nonfinite"] == 0), what
                assert got["converged"] == 1 and got["conv_eps"] == EPS and got["state_epoch"] == epochs[state], what
                assert np.all(got["max_abs_r"] < EPS) and np.all(got["max_abs_r"] > 0.0) and np.all(got["n_p_nonzero"] > 100), what
                # the row the device names holds, in numpy's evaluation, the device's maximum to rounding
                assert np.all(np.abs(want["err"][np.arange(n), got["inv_argmax"]] - got["inv_max_err"]) < INVARIANT_TOL), what
                runs.append(got)
            same_bits(runs[0], runs[3], (s.directed, state, n, "the plan's setting again"))
            for other in runs[1:3]:   # the residual part does not depend on the setting at all
                for k in EXACT:
                    assert np.asarray(runs[0][k]).tobytes() == np.asarray(other[k]).tobytes(), k
            dot = e.group_dot_dense_dev(gid, d_ones, 1)
            assert np.array_equal(bits(dot[0]), bits(runs[0]["sum_p"])), (state, n)
            # either part alone: the same values, the other part's names absent
            only_r, only_i = e.group_certify(gid, EPS, invariant=False), e.group_certify(gid, EPS, residual=False)
            assert "inv_max_err" not in only_r and "max_abs_r" not in only_i
            same_bits(only_r, {k: runs[0][k] for k in only_r}, "residual alone")
            same_bits(only_i, {k: runs[0][k] for k in only_i}, "invariant alone")
        # the conditions on the rig
        if not s.directed:
            assert deg.max() > 64, deg.max()             # an out-row longer than a wave
        assert np.any(-(-deg // 7) >= 3), deg.max()      # piece_edges = 7: a row of three pieces or more
    hip.free_all()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def slot_with_the_groups_state(directed=1, n_epochs=1):
    """An engine with a slot and a one-lane group of the same source; the slot is GIVEN the group's state (two solves of one source
    need not agree to the bit: tests/test_explain_gpu.py), the read back is asserted equal bit for bit."""
    V, e1, e2 = small_stream()
    e = eng.Engine(V, 600, directed, 20, schedule=eng.SCHEDULE_SYNC, n_epochs=n_epochs)
    e.load_window(e1[:600], e2[:600])
    src = int(datagen.top_sources(V, e1, e2, 600, directed, 1)[0])
    slot, gid = e.add_source(src), e.add_source_group([src])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    p, r = e.group_read(gid, 0)
    e.write(slot, p, r)
    p_slot, r_slot = e.read(slot)
    assert np.array_equal(bits(p_slot), bits(p)) and np.array_equal(bits(r_slot), bits(r))
    return e, slot, gid, src, p, r


def test_a_slot_equals_a_one_lane_group():
    e, slot, gid, src, p, r = slot_with_the_groups_state()
    tails, heads = edges_of(e)
    for piece, wave_rows in SETTINGS:
        e.debug_certify(piece, wave_rows)
        grp, want = check(e, gid, [src], EPS, ("one lane", piece, wave_rows), tails, heads)
        one = e.certify(slot, EPS)
        for k in RESIDUAL + ("inv_max_err", "inv_argmax"):   # value for value: a row of one double and a row of two are both one team's
            assert np.asarray(one[k]).tobytes() == np.asarray(grp[k]).tobytes(), k
        assert one["inv_max_err"][0] < INVARIANT_TOL and abs(one["inv_max_err"][0] - want["inv_max_err"][0]) < INVARIANT_TOL
        assert one["max_abs_r"].shape == (1,) and one["inv_argmax"].shape == (1,)
        assert (one["state_epoch"], one["converged"]) == (-2, 0) and grp["state_epoch"] >= 0 and grp["converged"] == 1   # (the write: unknown, unconverged)
        same_bits(one, e.certify(slot, EPS), ("slot again", piece, wave_rows))
    e.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_injected_residuals():
    e, slot, gid, src, p, r = slot_with_the_groups_state()
    V = e.V
    has_id = e.id_map() >= 0
    named = np.nonzero(has_id & (np.arange(V) != src))[0]
    v, v2, v3 = int(named[40]), int(named[7]), int(named[90])
    assert v2 < v < v3

    def with_r(changes, p_changes=()):
        r2, p2 = r.copy(), p.copy()
        for at, val in changes:
            r2[at] = val
        for at, val in p_changes:
            p2[at] = val
        e.write(slot, p2, r2)
        assert np.array_equal(e.id_map() >= 0, has_id)   # (a write names the vertices it gives a value: these had a name)
        got = e.certify(slot, EPS, invariant=False)
        same_residual(got, cr.residual([p2], [r2], EPS, has_id), changes)
        return got

    got = with_r([(v, 5 * EPS)])
    assert got["n_pos"][0] == 1 and got["n_neg"][0] == 0 and got["max_abs_r"][0] == 5 * EPS and got["argmax_r"][0] == v
    got = with_r([(v, -5 * EPS)])
    assert got["n_pos"][0] == 0 and got["n_neg"][0] == 1 and got["max_abs_r"][0] == 5 * EPS and got["argmax_r"][0] == v
    got = with_r([(v, EPS), (v3, -EPS)])                        # r == eps is not counted: the inequalities are strict
    assert got["n_pos"][0] == 0 and got["n_neg"][0] == 0 and got["max_abs_r"][0] == EPS and got["argmax_r"][0] == v
    got = with_r([(v, np.nextafter(EPS, 1)), (v3, -np.nextafter(EPS, 1))])
    assert got["n_pos"][0] == 1 and got["n_neg"][0] == 1
    got = with_r([(v, 3 * EPS), (v2, -3 * EPS), (v3, 3 * EPS)])  # equal |r|: the smallest id
    assert got["argmax_r"][0] == v2 and got["n_pos"][0] == 2 and got["n_neg"][0] == 1
    # a NaN in p and an inf in r: two rows that count in n_nonfinite alone; every other output is the reference's without them
    got = with_r([(v3, np.inf), (v2, 2 * EPS)], [(v, np.nan)])
    assert got["n_nonfinite"][0] == 2 and got["n_pos"][0] == 1 and got["argmax_r"][0] == v2 and got["max_abs_r"][0] == 2 * EPS
    clean_p, clean_r, without = p.copy(), r.copy(), has_id.copy()
    clean_r[v2] = 2 * EPS
    clean_p[v] = clean_r[v] = clean_p[v3] = clean_r[v3] = 0.0
    without[[v, v3]] = False
    clean = cr.residual([clean_p], [clean_r], EPS, without)
    assert clean["n_nonfinite"][0] == 0
    for k in RESIDUAL:
        if k != "n_nonfinite":
            assert np.asarray(got[k]).tobytes() == np.asarray(clean[k]).tobytes(), k
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_injected_invariant_violation():
    e, slot, gid, src, p, r = slot_with_the_groups_state()
    tails, heads = edges_of(e)
    V = e.V
    loops = np.zeros(V, dtype=bool)
    loops[tails[tails == heads]] = True
    indeg = np.bincount(heads, minlength=V)
    v = int(np.nonzero((indeg > 0) & ~loops & (np.arange(V) != src))[0][3])
    assert indeg[v] > 0 and not loops[v]          # in-neighbours and no self loop
    p2 = p.copy()
    p2[v] += 1e-6
    e.write(slot, p2, r)
    want = cr.certify(V, tails, heads, [p2], [r], [src], EPS, has_id=e.id_map() >= 0)
    assert abs(want["inv_max_err"][0] - 1e-6) < 1e-12 and want["inv_argmax"][0] == v
    # v wins: an in-neighbour u of v moves by 0.85 * 1e-6 * (copies of u -> v) / (d(u) + 1) < 1e-6
    assert np.sort(want["err"][0])[-2] < 0.86e-6
    for piece, wave_rows in SETTINGS:
        e.debug_certify(piece, wave_rows)
        got = e.certify(slot, EPS)
        assert got["inv_argmax"][0] == v, (piece, wave_rows, got["inv_argmax"], v)
        assert abs(got["inv_max_err"][0] - want["inv_max_err"][0]) < INVARIANT_TOL, (got["inv_max_err"], want["inv_max_err"])
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_the_wrong_epoch(directed):
    V, e1, e2 = small_stream()
    W, c = 600, 20
    g = orc.Graph(V, e1, e2, directed, W, c)
    e = eng.Engine(V, W, directed, c, n_epochs=2)
    e.load_window(*g.window_edges())
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 10)]
    gid = e.add_source_group(srcs)
    e.group_init_solve(gid, EPS)
    k = 0
    for _ in range(2):
        assert not g.stream_updates()
        g.inc_construct(1)
        b1, b2, ins = g.batch()
        e.set_batch(b1, b2, ins)
        k = e.slide(*g.new_stream())
        e.group_update(gid, EPS)
    changed = set(np.asarray(b1).tolist()) | (set() if directed else set(np.asarray(b2).tolist()))   # the tails of batch k
    ps, rs = group_cols(e, gid, 10)
    has_id = e.id_map() >= 0
    old = cr.certify(V, *edges_of(e, k - 1), ps, rs, srcs, EPS, has_id)
    print("directed", directed, "numpy on window k - 1:", old["inv_max_err"])
    assert np.all(old["inv_max_err"] > 1e-6)
    for piece, wave_rows in SETTINGS:
        e.debug_certify(piece, wave_rows)
        got = e.group_certify(gid, EPS, k - 1)
        assert got["state_epoch"] == k and got["converged"] == 1
        assert np.all(np.abs(got["inv_max_err"] - old["inv_max_err"]) < INVARIANT_TOL), (got["inv_max_err"], old["inv_max_err"])
        assert np.array_equal(got["inv_argmax"], old["inv_argmax"]) and all(int(u) in changed for u in got["inv_argmax"]), got["inv_argmax"]
        same_residual(got, old, ("the residual part does not read the graph", piece, wave_rows))
        # against epoch k, named or as the newest, the same state is healthy
        for epoch in (k, -1):
            fine, _ = check(e, gid, srcs, EPS, ("epoch", epoch, piece, wave_rows), *edges_of(e, k), epoch=epoch)
            assert np.all(fine["inv_max_err"] < INVARIANT_TOL) and fine["state_epoch"] == k
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 16])
def test_set_lanes(n):
    V, W, c, batches = 4096, 1500, 100, 3
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    rng = np.random.default_rng(40 + n)
    kinds = lane_kinds(V, e1, rng)
    sets = [kinds[(i + 1) % 5] for i in range(n)]
    sets[2] = (sets[2][0], sets[2][1] * 3.0)             # the 300 weights with sum(h) = 3: p, and with it its rounding, scales with sum(h)
    seeds = [list(zip(ids.tolist(), w.tolist())) for ids, w in sets]
    total = np.array([w.sum() for _, w in sets])
    tol = INVARIANT_TOL * np.maximum(1.0, total)
    assert total.max() > 2.9
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c)
    e.load_window(*g.window_edges())
    gid = e.add_target_group(sets)
    e.group_init_solve(gid, EPS)
    for b in range(batches + 1):
        if b:
            assert not g.stream_updates()
            g.inc_construct(1)
            e.set_batch(*g.batch())
            e.slide(*g.new_stream())
            e.group_update(gid, EPS)
        tails, heads = edges_of(e)
        for piece, wave_rows in SETTINGS[:3]:
            e.debug_certify(piece, wave_rows)
            got, _ = check(e, gid, seeds, EPS, ("sets", n, b, piece, wave_rows), tails, heads, tol)
            assert np.all(got["inv_max_err"] < tol), (got["inv_max_err"], tol)
            assert np.all(got["n_pos"] == 0) and np.all(got["n_neg"] == 0) and np.all(got["n_nonfinite"] == 0)
    # the reference is sensitive to the seed vector: with the weights of lane 0 and lane 1 exchanged it reports a violation
    ps, rs = group_cols(e, gid, n)
    wrong = cr.invariant(V, tails, heads, ps, rs, [seeds[1], seeds[0]] + seeds[2:])
    assert wrong["inv_max_err"][0] > 1e-3 and wrong["inv_max_err"][1] > 1e-3 and np.all(wrong["inv_max_err"][2:] < tol[2:])
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_parked_zone_is_counted():
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
    parked = np.nonzero(id_map >= V - sp["parked"])[0]
    assert len(parked) == sp["parked"] and np.any(id_map < 0)
    tails, heads = edges_of(e)
    for piece, wave_rows in SETTINGS[:3]:
        e.debug_certify(piece, wave_rows)
        got, want = check(e, gid, [0, 1, 2], EPS, ("churn", piece, wave_rows), tails, heads)
        assert np.all(got["inv_max_err"] < INVARIANT_TOL) and np.all(got["n_pos"] == 0) and np.all(got["n_neg"] == 0)
    ps, _ = group_cols(e, gid, 3)
    in_parked = sum(int(np.count_nonzero(p[parked])) for p in ps)
    assert in_parked > 0                                   # parked rows hold a p != 0: the counts above hold only with them counted
    live_only = [int(np.count_nonzero(np.where(np.isin(np.arange(V), parked), 0.0, p))) for p in ps]
    assert got["n_p_nonzero"].tolist() == [a + int(np.count_nonzero(p[parked])) for a, p in zip(live_only, ps)]
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
    dbls, ints, longs = np.full(8, 7.5), np.full(8, 77, dtype=np.int32), np.full(8, 777, dtype=np.int64)
    out = eng.CertifyOut()
    for name, ptr in eng.CertifyOut._fields_[:10]:
        arr = {eng.CertifyOut._dp: dbls, eng.CertifyOut._ip: ints, eng.CertifyOut._lp: longs}[ptr]
        setattr(out, name, arr.ctypes.data_as(ptr))
    out.state_epoch, out.converged, out.conv_eps = 55, 55, 55.0
    O = C.byref(out)

    def refused(epoch=-1, eps=EPS, flags=3, o=O, group=gid, slot_=slot):
        rcs = (L.dppr_group_certify(h, group, epoch, eps, flags, o), L.dppr_certify(h, slot_, epoch, eps, flags, o))
        untouched = np.all(dbls == 7.5) and np.all(ints == 77) and np.all(longs == 777)
        return rcs == (-1, -1) and bool(untouched) and (out.state_epoch, out.converged, out.conv_eps) == (55, 55, 55.0)

    for kw in (dict(o=None), dict(flags=0), dict(flags=4), dict(flags=-1), dict(eps=0.0), dict(eps=-EPS), dict(eps=float("nan")),
               dict(group=5, slot_=5), dict(group=-1, slot_=-1), dict(epoch=newest - 2), dict(epoch=newest + 1)):
        assert refused(**kw), list(kw)
    assert b"not resident" in L.dppr_last_error(h)
    for bad in ((-1, 0), (0, 3), (0, 128), (0, -1), ((1 << 20) + 1, 0)):
        with pytest.raises(eng.DpprError):
            e.debug_certify(*bad)
    # a call that asks for nothing writes the three words alone; a part whose pointers are all NULL is not run
    empty = eng.CertifyOut()
    assert L.dppr_group_certify(h, gid, -1, EPS, 3, C.byref(empty)) == 0
    assert (empty.state_epoch, empty.converged, empty.conv_eps) == (newest, 1, EPS)
    only = eng.CertifyOut()
    lens = np.full(2 + 3, 777, dtype=np.int64)
    only.n_p_nonzero = lens.ctypes.data_as(eng.CertifyOut._lp)
    assert L.dppr_group_certify(h, gid, newest - 1, EPS, 3, C.byref(only)) == 0   # (the older resident epoch: accepted)
    ps, _ = group_cols(e, gid, 2)
    assert lens[:2].tolist() == [np.count_nonzero(p) for p in ps] and np.all(lens[2:] == 777)
    only.inv_max_err = dbls.ctypes.data_as(eng.CertifyOut._dp)
    assert L.dppr_group_certify(h, gid, newest, EPS, eng.CERT_RESIDUAL, C.byref(only)) == 0 and np.all(dbls == 7.5)   # (the flag leaves the part out)
    assert np.all(ints == 77) and np.all(longs == 777)
    e.close()


def test_every_buffer_goes_with_the_engine():
    """On an engine whose scratch state another family has made already, as on a fresh one, the result is the reference's, the
    device time is reported, and all of the work space goes with the engine."""
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
        check(s.e, gid, s.srcs[:10], EPS, ("warm", warm), *edges_of(s.e))
        assert eng.live_bytes()[0] > held[0] and eng.live_bytes()[1] > held[1]   # (the block and its pinned twin are there)
        assert s.e.query_ms() > 0.0
        s.e.close()
    assert eng.live_bytes() == before
