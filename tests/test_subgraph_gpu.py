"""The subgraph a top-k order induces, built on the device (dppr_subgraph / dppr_group_subgraph), against the numpy restatement
of tests/subgraph_ref.py over what the engine reports through its other calls: the order and its p from topk / group_topk, the
rows from read_out_graph of the same epoch. Every comparison is exact: array_equal and the same dtypes, p by bit pattern. Every
result is also asked for with each row placed by the histogram kernel (wave_max = 0), and with the rows of more than 64 matches placed
by it, and must not change."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests import subgraph_ref
from tests.cf_stream import conflict_free_stream
from tests.test_changes_gpu import bits
from tests.test_cluster_gpu import rmat_window
from tests.test_conflict_free_streams import EPS as CF_EPS, SMALL
from tests.test_export_gpu import Hip
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 63, 64, 65, 1000, 8192)
CL_SPLIT = 2048  # entries of a row one wave walks (dppr_cluster_plan.hpp): a longer row is counted in pieces and placed by k_sg_long
EPS = 1e-7
NAMES = ("counts", "offsets", "ids", "p", "row_ptr", "col")


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def graph_of(e, epoch=-1):
    row, col = e.read_out_graph(epoch)
    return e.V, row, col


def topk_of(e, hd, k, min_p):
    return [e.topk(hd[1], k, min_p)[:2]] if hd[0] == "slot" else [t[:2] for t in e.group_topk(hd[1], k, min_p)]


def run(e, hd, k, min_p=0.0, epoch=-1):
    """The call as a group call: (counts [n], offsets [n + 1], ids [n][k], p [n][k], row_ptr [n][k + 1], col)."""
    if hd[0] == "group":
        return e.group_subgraph(hd[1], k, min_p, epoch)
    cnt, ids, p, row_ptr, col = e.subgraph(hd[1], k, min_p, epoch)
    return (np.array([cnt], dtype=np.int32), np.array([0, len(col)], dtype=np.int64), ids[None, :], p[None, :], row_ptr[None, :], col)


def same(got, want, tag):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, tag + (name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g) if name == "p" else g, bits(w) if name == "p" else w), tag + (name,)


def check(e, hd, graph, k, min_p=0.0, epoch=-1, what=""):
    """One call against the restatement, by the default fill and with every row through the histogram kernel; returns the result."""
    tops = topk_of(e, hd, k, min_p)
    cnt, off, ids, rp, col = subgraph_ref.subgraph(*graph, [t[0] for t in tops], k)
    p = np.zeros((len(tops), k))
    for i, t in enumerate(tops):
        p[i, :len(t[1])] = t[1]
    want = (cnt, off, ids, p, rp, col)
    tag = (what, hd, k, min_p)
    got = run(e, hd, k, min_p, epoch)
    same(got, want, tag)
    e.set_subgraph_wave_max(0)
    same(run(e, hd, k, min_p, epoch), want, tag + ("every row by the histogram",))
    e.set_subgraph_wave_max(64)
    same(run(e, hd, k, min_p, epoch), want, tag + ("rows of up to 64 matches by a wave",))
    e.set_subgraph_wave_max(256)  # (the default)
    return got


def rows_of(got, i):
    L = int(got[0][i])
    return [got[5][got[4][i, j]:got[4][i, j + 1]] for j in range(L)]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_equals_the_restatement(directed):
    e, srcs = rmat_window(directed)
    slot = e.add_source(srcs[0])
    gid = e.add_source_group(srcs[:3])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    graph = graph_of(e)
    assert max(len(t[0]) for t in topk_of(e, ("group", gid), 8192, 0.0)) < 8192  # the largest k exceeds the qualifying count
    for hd in (("slot", slot), ("group", gid)):
        for k in KS:
            for min_p in (0.0, 1e-6):
                got = check(e, hd, graph, k, min_p)
                assert got[4].shape == (len(got[0]), k + 1) and np.all(got[4][:, 0] == got[1][:-1]) and np.all(got[4][:, -1] == got[1][1:])
    # duplicates and self loops are really exercised: a row with a repeated position, a row that holds its own position
    got = run(e, ("group", gid), 1000)
    rows = [r for i in range(3) for r in rows_of(got, i)]
    own = [j for i in range(3) for j in range(int(got[0][i]))]
    assert any(np.any(np.diff(r) == 0) for r in rows) and any(j in r for j, r in zip(own, rows))
    assert all(np.all(np.diff(r) >= 0) for r in rows) and got[1][-1] > 100
    e.close()


# 2, 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [1, 0])
def test_ties_to_the_conductance_sweep_and_a_prefix_does_not_depend_on_what_follows(directed):
    """On the same state dppr_group_cluster reports vol[j] and cut_out[j] of every prefix S_j. vol counts every stored out-edge of
    S_j, a self loop included, and cut_out those that leave S_j, which a self loop never does: vol[j] - cut_out[j] is the number of
    stored edges inside S_j, self loops included, and that is the number of entries of rows <= j with a position <= j. (Counting
    the self loops off the left side would break the identity wherever S_j holds one: the window has one, and it is checked that the
    term matters.)"""
    e, srcs = rmat_window(directed)
    gid = e.add_source_group(srcs[:3])
    e.group_init_solve(gid, EPS)
    for k in (1000, 8192):
        got = run(e, ("group", gid), k)
        best, ids, cut_out, cut_in, vol = e.group_cluster(gid, k, profile=True)
        assert np.array_equal(ids, got[2])
        loops = 0
        for i in range(3):
            L = int(got[0][i])
            assert L == best[i]["count"] > 64
            inside = np.zeros(L, dtype=np.int64)   # entries (j, b) by max(j, b): the first prefix that holds both ends
            selfs = np.zeros(L, dtype=np.int64)
            for j, r in enumerate(rows_of(got, i)):
                np.add.at(inside, np.maximum(r, j), 1)
                selfs[j] += int(np.sum(r == j))
            assert np.array_equal(np.cumsum(inside), (vol[i] - cut_out[i])[:L]), (k, i)
            loops += int(selfs.sum())
        assert loops > 0
    # the prefix property between k = 64 and k = 1000
    short, long = run(e, ("group", gid), 64), run(e, ("group", gid), 1000)
    assert np.array_equal(short[2], long[2][:, :64]) and np.array_equal(bits(short[3]), bits(long[3][:, :64]))
    for i in range(3):
        assert long[0][i] > 64 == short[0][i]
        for a, b in zip(rows_of(short, i), rows_of(long, i)[:64]):
            assert np.array_equal(a, b[b < 64])
        assert sum(len(b) for b in rows_of(long, i)[:64]) > sum(len(a) for a in rows_of(short, i))  # (a proper restriction)
    e.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_group_width():
    e, srcs = rmat_window(1)
    graph = graph_of(e)
    for n in (1, 2, 5, 10, 16):
        gid = e.add_source_group(srcs[:n])
        e.group_init_solve(gid, EPS)
        for k in (65, 8192):
            got = check(e, ("group", gid), graph, k, what=f"n={n}")
            assert got[2].shape == (n, k) and got[4].shape == (n, k + 1) and len(got[1]) == n + 1
    e.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_rows_counted_in_pieces_and_placed_by_the_histogram():
    """The star of tests/test_cluster_gpu.py: a hub of CL_SPLIT + 300 leaves on an undirected window, a few hundred edges among the
    leaves, a path hanging off leaf 1 -- and one hub-leaf edge stored twice, so the long row holds a multiplicity. Sources: the hub
    (the long row at position 0) and the far end of the path (the hub deep in the order)."""
    text = open(os.path.join(ROOT, "dynamicppr_amd", "csrc", "dppr_cluster_plan.hpp")).read()
    assert int(re.search(r"constexpr int CL_SPLIT = (\d+);", text).group(1)) == CL_SPLIT
    leaves, path = CL_SPLIT + 300, 6
    rng = np.random.default_rng(17)
    a, b = rng.integers(1, leaves + 1, 400), rng.integers(1, leaves + 1, 400)
    chain = np.arange(leaves + 1, leaves + 1 + path)
    w1 = np.concatenate([np.zeros(leaves, dtype=np.int64), [0], a, [1], chain[:-1]]).astype(np.int32)
    w2 = np.concatenate([np.arange(1, leaves + 1), [7], b, [chain[0]], chain[1:]]).astype(np.int32)
    perm = rng.permutation(len(w1))
    V, far = 4096, int(chain[-1])
    e = eng.Engine(V, len(w1), 0, 1)
    e.load_window(w1[perm], w2[perm])
    graph = graph_of(e)
    deg = np.diff(graph[1])
    assert deg[0] == leaves + 1 > CL_SPLIT and np.sort(deg)[-2] < 64
    gid = e.add_source_group([0, far])
    slot = e.add_source(far)
    e.group_init_solve(gid, 1e-9)
    e.init_solve(slot, 1e-9)
    for k in (1, 5, 1000, 8192):
        got = check(e, ("group", gid), graph, k)
        check(e, ("slot", slot), graph, k)
        assert got[2][0, 0] == 0
        if k >= 1000:
            hub_row = rows_of(got, 0)[0]
            assert len(hub_row) > 900 and np.all(np.diff(hub_row) >= 0)
            if k == 8192:  # the whole star: the row is longer than one chunk, every leaf once and leaf 7 twice
                assert 7 in got[2][0] and len(hub_row) > CL_SPLIT and np.sum(np.diff(hub_row) == 0) == 1
            at = int(np.nonzero(got[2][1] == 0)[0][0])
            assert 3 <= at < 100 and len(rows_of(got, 1)[at]) > 900, at
    e.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_capacity(hip):
    e, srcs = rmat_window(1)
    gid = e.add_source_group(srcs[:3])
    e.group_init_solve(gid, EPS)
    L, h, k, n = e._L, e._h, 1000, 3
    want = run(e, ("group", gid), k)
    total = int(want[1][n])
    assert total > 10
    cnt, off = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int64)
    # the size query with NULL arrays
    assert L.dppr_group_subgraph(h, gid, -1, k, 0.0, 0, eng.DEST_HOST, cnt.ctypes.data, off.ctypes.data, None, None, None, None) == 0
    assert np.array_equal(off, want[1]) and np.array_equal(cnt, want[0])
    for dest in (eng.DEST_HOST, eng.DEST_DEVICE):
        for cap, filled in ((total - 1, False), (total, True), (total + 5, True)):
            cnt[:], off[:] = -1, -1
            col = np.full(total + 5, -77, dtype=np.int32)
            rp = np.full((n, k + 1), -77, dtype=np.int64)
            d_col, d_rp = hip.alloc(4 * (total + 5)), hip.alloc(rp.nbytes)
            dev = dest == eng.DEST_DEVICE
            assert L.dppr_group_subgraph(h, gid, -1, k, 0.0, cap, dest, cnt.ctypes.data, off.ctypes.data, None, None,
                                         d_rp if dev else rp.ctypes.data, d_col if dev else col.ctypes.data) == 0
            assert np.array_equal(off, want[1]) and np.array_equal(cnt, want[0]), (dest, cap)  # the true counts either way
            if dev:
                col, rp = hip.read(d_col, 4 * (total + 5), np.int32), hip.read(d_rp, rp.nbytes, np.int64).reshape(n, k + 1)
            pad = -77 if not dev else np.frombuffer(b"\xab" * 4, dtype=np.int32)[0]
            assert np.array_equal(rp, want[4]), (dest, cap)
            if filled:
                assert np.array_equal(col[:total], want[5]) and np.all(col[total:] == pad), (dest, cap)
            else:
                assert np.all(col == pad), (dest, cap)
            hip.free_all()
    e.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_after_slides_renumberings_and_on_the_right_epoch_only():
    V, W, c, batches = 4096, 1500, 100, 60
    e1, e2 = churn_stream(V, W + (batches + 8) * c, 400, 5)
    g = orc.Graph(V, e1, e2, 1, W, c)
    e = eng.Engine(V, W, 1, c, n_epochs=2)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    slot = e.add_source(0)
    gid = e.add_source_group([0, 1, 2])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    done, newest, renumbered = 0, 0, True
    while done < batches or renumbered:  # (a renumbering drops the older epoch: end on a slide that kept it)
        assert done < batches + 8 and not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        before = e.id_space()["renumberings"]
        newest = e.slide(*g.new_stream())
        e.update(slot, EPS)
        e.group_update(gid, EPS)
        renumbered = e.id_space()["renumberings"] > before
        done += 1
    sp = e.id_space()
    assert sp["parked"] > 0 and sp["renumberings"] > 0, sp
    graph = graph_of(e)
    in_window = np.zeros(V, dtype=bool)
    w1, w2 = g.window_edges()
    in_window[w1] = in_window[w2] = True
    for hd in (("slot", slot), ("group", gid)):
        for k in (100, 8192):
            got = check(e, hd, graph, k, what="after slides")
        for i in range(got[2].shape[0]):  # a parked vertex (no edge in the window, p > 0) inside the order: an empty row, never a head
            ids = got[2][i][got[2][i] >= 0]
            at = np.nonzero(~in_window[ids])[0]
            assert len(at) and at[0] > 0
            rows = rows_of(got, i)
            assert len(rows[at[0]]) == 0 and not any(at[0] in r for r in rows)
    # the states stand on the newest epoch: the older one is resident but refused, an evicted one is no epoch at all
    L, h = e._L, e._h
    cnt, off = np.full(3, 7, dtype=np.int32), np.full(4, 7, dtype=np.int64)
    ids, p, rp = np.full(3 * 16, 7, dtype=np.int32), np.full(3 * 16, 2.5), np.full(3 * 17, 7, dtype=np.int64)

    def rcs(epoch):
        a = (epoch, 16, 0.0, 0, eng.DEST_HOST, cnt.ctypes.data, off.ctypes.data, ids.ctypes.data, p.ctypes.data, rp.ctypes.data, None)
        return L.dppr_subgraph(h, slot, *a), L.dppr_group_subgraph(h, gid, *a)

    def untouched():
        return np.all(cnt == 7) and np.all(off == 7) and np.all(ids == 7) and np.all(p == 2.5) and np.all(rp == 7)

    e.read_out_graph(newest - 1)  # (resident)
    assert rcs(newest - 1) == (-1, -1) and untouched()
    assert b"another epoch" in L.dppr_last_error(h)
    assert rcs(newest - 2) == (-1, -1) and rcs(newest + 1) == (-1, -1) and untouched()
    assert b"not resident" in L.dppr_last_error(h)
    assert rcs(newest) == (0, 0) and not untouched()
    # a state set by dppr_write stands on no epoch in particular: any resident one is accepted
    pp, rr = e.read(slot)
    e.write(slot, pp, rr)
    for epoch in (newest - 1, newest, -1):
        check(e, ("slot", slot), graph_of(e, epoch), 8192, epoch=epoch, what=f"written, epoch {epoch}")
    assert L.dppr_subgraph(h, slot, newest - 2, 16, 0.0, 0, eng.DEST_HOST, cnt.ctypes.data, off.ctypes.data, None, None, None, None) == -1
    e.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(hip):
    e, srcs = rmat_window(1)
    slot = e.add_source(srcs[0])
    gid = e.add_source_group(srcs[:2])
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    L, h, n, k = e._L, e._h, 2, 8
    total = int(run(e, ("group", gid), k)[1][n])
    assert total > 1
    cnt, off = np.empty(n, dtype=np.int32), np.empty(n + 1, dtype=np.int64)
    ids, p, rp, col = np.empty(n * k, dtype=np.int32), np.empty(n * k), np.empty(n * (k + 1), dtype=np.int64), np.empty(total, dtype=np.int32)
    sizes = dict(ids=4 * n * k, p=8 * n * k, rp=8 * n * (k + 1), col=4 * total)
    d = {name: hip.alloc(nb) for name, nb in sizes.items()}
    short = {name: hip.alloc(nb - (8 if name in ("p", "rp") else 4)) for name, nb in sizes.items()}

    def fill():
        cnt[:], off[:], ids[:], p[:], rp[:], col[:] = 7, 7, 7, 2.5, 7, 7

    def untouched():
        host = np.all(cnt == 7) and np.all(off == 7) and np.all(ids == 7) and np.all(p == 2.5) and np.all(rp == 7) and np.all(col == 7)
        dev = all(np.all(hip.read(d[name], nb) == 0xAB) for name, nb in sizes.items())
        return host and dev and all(np.all(hip.read(short[name], nb - 8) == 0xAB) for name, nb in sizes.items())

    H, D = eng.DEST_HOST, eng.DEST_DEVICE
    CN, OF, I, P, R, CO = cnt.ctypes.data, off.ctypes.data, ids.ctypes.data, p.ctypes.data, rp.ctypes.data, col.ctypes.data

    def rcs(slot_=None, gid_=None, epoch=-1, k_=k, min_p=0.0, cap=total, dest=H, cn=CN, of=OF, i=I, p_=P, r=R, co=CO, only=None):
        a = (epoch, k_, min_p, cap, dest, cn, of, i, p_, r, co)
        calls = (lambda: L.dppr_subgraph(h, slot if slot_ is None else slot_, *a), lambda: L.dppr_group_subgraph(h, gid if gid_ is None else gid_, *a))
        return tuple(f() for f in calls) if only is None else calls[only]()  # (only: a slot needs less of every section than the group)

    fill()
    assert rcs(only=1) == 0 and not untouched()  # (the call as such is fine)
    fill()
    for bad_k in (0, -1, eng.SUBGRAPH_MAX + 1, 2**31 - 1):
        assert rcs(k_=bad_k) == (-1, -1) and untouched(), bad_k
    for min_p in (-1e-300, -1.0, float("nan"), float("-inf")):
        assert rcs(min_p=min_p) == (-1, -1) and untouched(), min_p
    assert rcs(cap=-1) == (-1, -1) and rcs(cap=1, co=None) == (-1, -1) and rcs(cap=total, co=None, dest=D) == (-1, -1) and untouched()
    assert rcs(of=None) == (-1, -1) and rcs(cn=None) == (-1, -1) and rcs(of=None, cap=0, co=None) == (-1, -1) and untouched()
    assert rcs(dest=2) == (-1, -1) and rcs(dest=-1) == (-1, -1) and untouched()
    assert rcs(slot_=5, gid_=5) == (-1, -1) and rcs(slot_=-1, gid_=-1) == (-1, -1) and untouched()
    assert rcs(epoch=1) == (-1, -1) and rcs(epoch=7) == (-1, -1) and untouched()
    # a device destination: a host pointer, one element too short, misaligned, past the end of its allocation -- section by section
    good = dict(i=d["ids"], p_=d["p"], r=d["rp"], co=d["col"])
    for arg, name, host_ptr in (("i", "ids", I), ("p_", "p", P), ("r", "rp", R), ("co", "col", CO)):
        step = 8 if name in ("p", "rp") else 4
        for ptr in (host_ptr, short[name], d[name] + step // 2, d[name] + step):
            assert rcs(dest=D, only=1, **{**good, arg: ptr}) == -1 and untouched(), (name, ptr - d[name])
    # the limits themselves are fine, and so are the buffers for the calls that fit them
    for kk in (1, eng.SUBGRAPH_MAX):
        assert L.dppr_subgraph(h, slot, -1, kk, 0.0, 0, H, CN, OF, None, None, None, None) == 0
        assert L.dppr_group_subgraph(h, gid, 0, kk, 0.0, 0, D, CN, OF, None, None, None, None) == 0
    assert L.dppr_group_subgraph(h, gid, -1, k, 0.0, total, D, CN, OF, d["ids"], d["p"], d["rp"], d["col"]) == 0 and off[n] == total
    want = run(e, ("group", gid), k)
    assert np.array_equal(hip.read(d["col"], 4 * total, np.int32), want[5]) and np.array_equal(hip.read(d["ids"], 4 * n * k, np.int32), want[2].ravel())
    assert np.array_equal(hip.read(d["rp"], 8 * n * (k + 1), np.int64), want[4].ravel())
    assert np.array_equal(hip.read(d["p"], 8 * n * k, np.uint64), bits(want[3]).ravel())
    e.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_no_side_effects():
    """p and r read back bit-identical after the calls, the time of the last query is reported, and the next group_update gives
    the same bits as on an engine that never asked. The stream is a conflict-free one (tests/cf_stream.py), as in
    tests/test_cluster_gpu.py: two engines that do the same give the same bits there, and a difference is the query's doing."""
    V, e1, e2, meta = conflict_free_stream(seed=1, **SMALL)
    W, c = SMALL["W"], SMALL["c"]
    sources = [int(x) for x in meta["sources"][:3]]
    states = []
    for ask in (True, False):
        g = orc.Graph(V, e1, e2, 1, W, c)
        e = eng.Engine(V, W, 1, c)
        e.load_window(*g.window_edges())
        gid = e.add_source_group(sources)
        slot = e.add_source(sources[0])
        e.group_init_solve(gid, CF_EPS)
        e.init_solve(slot, CF_EPS)
        reads = []
        for step in range(3):
            if ask:
                before = [e.group_read(gid, i) for i in range(3)] + [e.read(slot)]
                e.set_profiling(1)
                got = e.group_subgraph(gid, 8192)
                assert e.query_ms() > 0 and np.all(got[0] > 1)
                e.subgraph(slot, 1000, 1e-12)
                assert e.query_ms() > 0
                e.set_profiling(0)
                after = [e.group_read(gid, i) for i in range(3)] + [e.read(slot)]
                for x, y in zip(before, after):
                    assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1]))
            assert not g.stream_updates()
            g.inc_construct(1)
            e.set_batch(*g.batch())
            e.slide(*g.new_stream())
            e.group_update(gid, CF_EPS)
            e.update(slot, CF_EPS)
            reads += [e.group_read(gid, i) for i in range(3)] + [e.read(slot)]
        states.append(reads)
        e.close()
    assert any(np.any(x[0] != y[0]) for x, y in zip(states[0][:4], states[0][4:8]))  # (the batches move the states)
    for x, y in zip(*states):
        assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1]))
