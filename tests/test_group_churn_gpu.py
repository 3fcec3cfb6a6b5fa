"""Sources of a running source group are replaced, added and dropped (dppr_group_replace_source, dppr_group_add_source,
dppr_group_remove_source, dppr_group_sources; include/dppr.h) while the stream goes on. The new column is solved from scratch
on the epoch the group stands on, at the group's tolerance; every lane must equal the oracle's synchronous schedule (group
iterations are sweeps) after every such call and after every later update, the other lanes must not change by a bit, and the
work counted over a call must be exactly the new column's -- which is what proves that no other column pushed."""
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_engine_gpu import SYNC_TOL
from tests.test_renumbering_gpu import churn_stream
from tests.test_topk_gpu import check_group

pytestmark = pytest.mark.gpu

SMALL = dict(W=600, c=20, eps=1e-9)
COUNTED = ("batches", "records", "gpu_ms")  # describe dppr_group_update: a change of the sources leaves them alone


def small_stream():
    return datagen.rmat_stream(9, 6000, 11)


def ranked_sources(V, e1, e2, W, directed, n=24):
    return [int(s) for s in datagen.top_sources(V, e1, e2, W, directed, n)]


class Driver:
    """A source group and one oracle state per lane over the same stream (the pattern of run_source_group)."""

    def __init__(self, V, e1, e2, W, c, eps, directed, sources, tuning=None, resident=True, push=None, n_epochs=1, renumbering=None):
        self.V, self.eps = V, eps
        self.e = eng.Engine(V, W, directed, c, n_epochs=n_epochs, **(tuning or {}))
        self.e.set_group_resident(resident)
        if push is not None:
            self.e.set_group_push(*push)
        if renumbering is not None:
            self.e.set_renumbering(*renumbering)
        self.g = orc.Graph(V, e1, e2, directed, W, c)
        self.sources = [int(s) for s in sources]
        self.states = [orc.State(V, s, eps) for s in self.sources]
        self.e.load_window(*self.g.window_edges())
        self.gid = self.e.add_source_group(self.sources)
        for s in self.states:
            s.sync_execute(self.g)
        self.e.group_init_solve(self.gid, eps)
        self.check("from scratch")

    def close(self):
        self.e.close()

    def dense(self):
        return [self.e.group_read(self.gid, i) for i in range(len(self.sources))]

    def check(self, what):
        assert self.e.group_sources(self.gid) == self.sources, what
        for i, s in enumerate(self.states):
            p, r = self.e.group_read(self.gid, i)
            dp, dr = np.max(np.abs(p - s.p)), np.max(np.abs(r - s.r))
            assert dp < SYNC_TOL and dr < SYNC_TOL, (what, i, dp, dr)
            assert np.max(np.abs(r)) <= self.eps, (what, i)
        with pytest.raises(eng.DpprError):
            self.e.group_read(self.gid, len(self.sources))

    def batches(self, k, epoch=-1):
        for _ in range(k):
            assert not self.g.stream_updates()
            self.g.inc_construct(1)
            self.e.set_batch(*self.g.batch())
            self.e.slide(*self.g.new_stream())
            self.follow(epoch)

    def follow(self, epoch=-1):
        """the group and the oracle states take the batch the oracle graph stands on"""
        for s in self.states:
            s.sync_inc_execute(self.g)
        self.e.group_update(self.gid, self.eps, epoch)
        self.check("update")

    def churn(self, op, index=None, source=None):
        """One call; `kept`: old lane of every lane that stays, in the new order."""
        n = len(self.sources)
        before, st0 = self.dense(), self.e.group_stats(self.gid)
        if op == "replace":
            ms = self.e.group_replace_source(self.gid, index, source)
            kept = [(i, i) for i in range(n) if i != index]
            self.sources[index] = int(source)
        elif op == "add":
            index, ms = self.e.group_add_source(self.gid, source)
            assert index == n
            kept = [(i, i) for i in range(n)]
            self.sources.append(int(source))
            self.states.append(None)
        else:
            self.e.group_remove_source(self.gid, index)
            ms = None
            kept = [(i, i if i < index else i - 1) for i in range(n) if i != index]
            del self.sources[index]
            del self.states[index]
        st1 = self.e.group_stats(self.gid)
        for k in COUNTED:
            assert st1[k] == st0[k], (op, k)
        if op == "remove":
            want = {"F": 0, "E": 0}
        else:
            assert ms > 0
            fresh = orc.State(self.V, int(source), self.eps)
            fresh.sync_execute(self.g)  # from scratch on the window the group stands on
            self.states[index] = fresh
            want = fresh.stats()
        assert st1["sum_F"] - st0["sum_F"] == want["F"], (op, n, index)  # no other column pushed
        assert st1["sum_E"] - st0["sum_E"] == want["E"], (op, n, index)
        after = self.dense()
        for old, new in kept:
            assert np.array_equal(before[old][0], after[new][0]) and np.array_equal(before[old][1], after[new][1]), (op, old, new)
        self.check(op)
        return ms


@pytest.mark.parametrize("n", [1, 2, 5, 8, 10, 16])
@pytest.mark.parametrize("directed", [1, 0])
def test_replace_first_and_last_lane(directed, n):
    V, e1, e2 = small_stream()
    ranked = ranked_sources(V, e1, e2, SMALL["W"], directed)
    d = Driver(V, e1, e2, directed=directed, sources=ranked[:n], **SMALL)
    d.batches(1)
    d.churn("replace", 0, ranked[16])
    d.batches(2)
    d.churn("replace", n - 1, ranked[17])
    d.batches(2)
    d.churn("replace", n - 1, ranked[17])        # the same vertex again: a re-solve of that lane
    d.churn("replace", 0, d.sources[n - 1])      # a duplicate of another lane
    d.batches(3)
    assert d.e.group_stats(d.gid)["batches"] == 8
    d.close()


@pytest.mark.parametrize("chain", [(1, 4), (7, 9), (15, 16)], ids=["1-2-3-4", "7-8-9", "15-16"])
@pytest.mark.parametrize("directed", [1, 0])
def test_add_sources_along_every_kind_of_step(directed, chain):
    """1 -> 2 and 7 -> 8 fill the padding lane (no relayout), 2 -> 3 doubles the row, 3 -> 4 fills, 8 -> 9 switches to two doubles
    per lane (sweep groups re-cut to 512 vertices), 15 -> 16 fills the last lane; a 17th source is refused."""
    V, e1, e2 = small_stream()
    ranked = ranked_sources(V, e1, e2, SMALL["W"], directed)
    first, last = chain
    d = Driver(V, e1, e2, directed=directed, sources=ranked[:first], **SMALL)
    for n in range(first, last):
        d.batches(2)
        d.churn("add", source=ranked[n])
    d.batches(3)
    if last == 16:
        before = d.dense()
        with pytest.raises(eng.DpprError):
            d.e.group_add_source(d.gid, ranked[16])
        for (p0, r0), (p1, r1) in zip(before, d.dense()):
            assert np.array_equal(p0, p1) and np.array_equal(r0, r1)
        d.check("after a refused add")
    d.close()


@pytest.mark.parametrize("first,lanes", [(16, ["first"]), (9, ["middle"]), (3, ["last", "first"])], ids=["16-15", "9-8", "3-2-1"])
@pytest.mark.parametrize("directed", [1, 0])
def test_remove_sources_first_middle_last(directed, first, lanes):
    """16 -> 15 shifts inside the same width, 9 -> 8 goes back to one double per lane (beside tables cut for a wide group),
    3 -> 2 -> 1 halves the row and then leaves a padding lane; the last source cannot be removed."""
    V, e1, e2 = small_stream()
    ranked = ranked_sources(V, e1, e2, SMALL["W"], directed)
    d = Driver(V, e1, e2, directed=directed, sources=ranked[:first], **SMALL)
    for where in lanes:
        d.batches(2)
        n = len(d.sources)
        d.churn("remove", {"first": 0, "middle": n // 2, "last": n - 1}[where])
    d.batches(3)
    if len(d.sources) == 1:
        with pytest.raises(eng.DpprError):
            d.e.group_remove_source(d.gid, 0)
        d.check("after a refused remove")
        d.churn("add", source=ranked[20])       # and the group grows again
        d.batches(1)
    d.close()


@pytest.mark.parametrize("mode", ["multi-sweep", "one-launch-per-sweep", "tail-as-pushes", "rollcall-fails"])
def test_launch_forms_of_the_column_solve(mode):
    """The column's loop as multi-sweep resident launches (the default on a window whose sweep groups are all resident), as one
    launch per sweep, with its tail as pushes, and with a roll-call that cannot succeed."""
    V, e1, e2 = datagen.rmat_stream(12, 40000, 7)
    W, c, directed = 12000, 120, 0
    ranked = ranked_sources(V, e1, e2, W, directed)
    tuning = dict(persist_timeout_us=-1) if mode == "rollcall-fails" else None
    push = (10**9, 0) if mode == "tail-as-pushes" else None
    d = Driver(V, e1, e2, W, c, 1e-9, directed, ranked[:10], tuning=tuning, resident=mode not in ("one-launch-per-sweep", "tail-as-pushes"),
               push=push)
    d.batches(1)
    st0 = d.e.group_stats(d.gid)
    d.churn("replace", 3, ranked[16])
    d.churn("add", source=ranked[17])
    st = d.e.group_stats(d.gid)
    if mode == "multi-sweep":
        assert st["persist_launches"] > st0["persist_launches"] and st["persist_aborts"] == 0
    elif mode == "rollcall-fails":
        assert st["persist_aborts"] == 1
    else:
        assert st["persist_launches"] == 0
        if mode == "tail-as-pushes":
            assert st["pull_iterations"] < st["iterations"]
    d.batches(2)
    d.close()


def test_new_source_without_an_edge_or_an_id():
    """A vertex the window has never seen: it receives an internal id beyond every epoch's tables, which are re-cut."""
    V, e1, e2 = datagen.rmat_stream(10, 8000, 9)
    W, c, directed = 500, 10, 1
    used = set(e1[:W + 60 * c].tolist()) | set(e2[:W + 60 * c].tolist())
    lonely = [v for v in range(V) if v not in used][:2]
    top = ranked_sources(V, e1, e2, W, directed, 4)
    d = Driver(V, e1, e2, W, c, 1e-9, directed, top[:3])
    d.batches(1)
    ids = d.e.id_space()["ids"]
    d.churn("replace", 1, lonely[0])
    assert d.e.id_space()["ids"] == ids + 1
    d.batches(2)
    ids = d.e.id_space()["ids"]  # (the two slides brought vertices of their own)
    d.churn("add", source=lonely[1])
    assert d.e.id_space()["ids"] == ids + 1
    d.batches(3)
    d.close()


def test_parked_vertex_comes_back_as_a_source_and_a_dropped_one_is_parked():
    """On a stream that churns through the id range. Two vertices that the first window holds and the stream never names again:
    one is a source and is dropped (then a renumbering parks it -- a source never is), the other is parked as soon as its edges
    have left. Both come back as sources, revived from the parked zone: one added, one replacing."""
    V, W, c, eps, directed, batches = 4096, 1500, 100, 1e-9, 1, 60
    e1, e2 = churn_stream(V, W + batches * c, 400, 5)
    later = set(e1[W:].tolist()) | set(e2[W:].tolist())
    gone = [int(v) for v in dict.fromkeys(e1[:W].tolist() + e2[:W].tolist()) if v > 3 and v not in later]
    was_source, never_source = gone[0], gone[1]
    d = Driver(V, e1, e2, W, c, eps, directed, [0, 1, was_source, 2], renumbering=(1, 10, 16))
    d.batches(1)
    d.churn("remove", 2)
    d.batches(W // c)  # the first window has left
    seen = d.e.id_space()["renumberings"]
    for _ in range(25):
        d.batches(1)
        if d.e.id_space()["renumberings"] > seen:
            break
    sp = d.e.id_space()
    assert sp["renumberings"] > seen and sp["parked"] >= 2, sp
    d.churn("add", source=never_source)
    sp2 = d.e.id_space()
    assert sp2["revivals"] == sp["revivals"] + 1 and sp2["parked"] == sp["parked"] - 1, (sp, sp2)
    d.batches(2)
    sp2 = d.e.id_space()
    d.churn("replace", 0, was_source)
    sp3 = d.e.id_space()
    assert sp3["revivals"] == sp2["revivals"] + 1, (sp2, sp3)  # it was parked: a dropped source is no longer pinned as live
    d.batches(3)
    d.close()


def test_lagging_group_is_solved_on_its_own_epoch():
    """n_epochs = 3, two slides pre-staged: the column is solved on the epoch the group was last solved on, two and one epochs
    behind the newest, and the updates that follow in sequence match. A group that was never solved and one whose epoch
    the ring has overwritten are refused."""
    V, e1, e2 = small_stream()
    directed = 0
    ranked = ranked_sources(V, e1, e2, SMALL["W"], directed)
    d = Driver(V, e1, e2, directed=directed, sources=ranked[:5], n_epochs=3, **SMALL)
    feed = orc.Graph(V, e1, e2, directed, SMALL["W"], SMALL["c"])  # runs ahead of d.g, which stays where the group stands

    def stage():
        assert not feed.stream_updates()
        feed.inc_construct(1)
        d.e.set_batch(*feed.batch())
        return d.e.slide(*feed.new_stream())

    def catch_up(epoch):
        assert not d.g.stream_updates()
        d.g.inc_construct(1)
        d.follow(epoch)

    assert stage() == 1 and stage() == 2
    d.churn("replace", 1, ranked[16])  # on epoch 0, two behind
    catch_up(1)
    d.churn("replace", 4, ranked[17])  # on epoch 1, one behind
    d.churn("add", source=ranked[18])
    catch_up(2)
    d.churn("remove", 0)
    unsolved = d.e.add_source_group(ranked[:3])
    with pytest.raises(eng.DpprError):
        d.e.group_replace_source(unsolved, 0, ranked[19])
    with pytest.raises(eng.DpprError):
        d.e.group_add_source(unsolved, ranked[19])
    with pytest.raises(eng.DpprError):
        d.e.group_remove_source(unsolved, 0)
    assert d.e.group_sources(unsolved) == ranked[:3]
    assert stage() == 3
    catch_up(3)
    for k in (4, 5, 6):
        assert stage() == k   # epoch 3 leaves the ring of three
    before = d.dense()
    for call in (lambda: d.e.group_replace_source(d.gid, 0, ranked[19]), lambda: d.e.group_add_source(d.gid, ranked[19]),
                 lambda: d.e.group_remove_source(d.gid, 0)):
        with pytest.raises(eng.DpprError):
            call()
    assert d.e.group_sources(d.gid) == d.sources
    for (p0, r0), (p1, r1) in zip(before, d.dense()):
        assert np.array_equal(p0, p1) and np.array_equal(r0, r1)
    d.close()


def test_queries_after_a_change_of_the_sources():
    """group_topk returns exactly the new n rows, equal to numpy over the dense reads; group_read_at has the new shape."""
    V, e1, e2 = small_stream()
    directed = 0
    ranked = ranked_sources(V, e1, e2, SMALL["W"], directed)
    d = Driver(V, e1, e2, directed=directed, sources=ranked[:10], **SMALL)
    ids = np.array(ranked[:7] + [0, V - 1], dtype=np.int32)

    def queries(n):
        assert len(d.sources) == n
        dense = check_group(d.e, d.gid, n, ks=(10,), min_ps=(0.0,))
        p, r = d.e.group_read_at(d.gid, ids)
        assert p.shape == (len(ids), n) and r.shape == (len(ids), n)
        for i, (dp, dr) in enumerate(dense):
            assert np.array_equal(p[:, i], dp[ids]) and np.array_equal(r[:, i], dr[ids])

    queries(10)
    d.churn("add", source=ranked[16])
    queries(11)
    d.batches(1)
    d.churn("remove", 4)
    d.churn("remove", 0)
    queries(9)
    d.churn("replace", 8, ranked[17])
    queries(9)
    d.close()


def test_rejected_calls_change_nothing():
    V, e1, e2 = datagen.rmat_stream(10, 8000, 9)
    W, c, directed = 500, 10, 1
    used = set(e1[:W + 60 * c].tolist()) | set(e2[:W + 60 * c].tolist())
    lonely = [v for v in range(V) if v not in used][0]  # would receive an id if a call got that far
    top = ranked_sources(V, e1, e2, W, directed, 20)
    d = Driver(V, e1, e2, W, c, 1e-9, directed, top[:3])
    full = d.e.add_source_group(top[:16])
    d.e.group_init_solve(full, 1e-9)
    one = d.e.add_source_group(top[:1])
    d.e.group_init_solve(one, 1e-9)
    unsolved = d.e.add_source_group(top[:2])
    d.batches(1)  # (d.gid moves on: `full`, `one` stay converged on epoch 0, which is gone from the ring of one)
    e = d.e

    def snapshot():
        return (e.group_sources(d.gid), e.group_sources(full), e.group_sources(one), e.group_sources(unsolved), e.id_space(),
                eng.live_bytes(), d.dense())

    before = snapshot()
    calls = [lambda: e.group_replace_source(99, 0, lonely), lambda: e.group_replace_source(-1, 0, lonely),
             lambda: e.group_add_source(99, lonely), lambda: e.group_remove_source(99, 0), lambda: e.group_sources(99),
             lambda: e.group_replace_source(d.gid, 3, lonely), lambda: e.group_replace_source(d.gid, -1, lonely),
             lambda: e.group_remove_source(d.gid, 3), lambda: e.group_remove_source(d.gid, -1),
             lambda: e.group_replace_source(d.gid, 0, V), lambda: e.group_replace_source(d.gid, 0, -1),
             lambda: e.group_add_source(d.gid, V), lambda: e.group_add_source(d.gid, -1),
             lambda: e.group_add_source(unsolved, lonely), lambda: e.group_replace_source(unsolved, 0, lonely),   # not converged
             lambda: e.group_remove_source(unsolved, 0),
             lambda: e.group_add_source(one, lonely), lambda: e.group_replace_source(full, 0, lonely)]            # their epoch is gone
    for i, call in enumerate(calls):
        with pytest.raises(eng.DpprError):
            call()
        after = snapshot()
        assert after[:6] == before[:6], i
        for (p0, r0), (p1, r1) in zip(before[6], after[6]):
            assert np.array_equal(p0, p1) and np.array_equal(r0, r1), i
    d.batches(1)
    d.close()


def test_full_and_single_groups_refuse_add_and_remove():
    """add at 16 sources and remove at 1 source on groups that are otherwise in order (converged, epoch resident)."""
    V, e1, e2 = small_stream()
    ranked = ranked_sources(V, e1, e2, SMALL["W"], 1)
    d = Driver(V, e1, e2, directed=1, sources=ranked[:16], **SMALL)
    one = d.e.add_source_group(ranked[:1])
    d.e.group_init_solve(one, SMALL["eps"])
    mem = eng.live_bytes()
    with pytest.raises(eng.DpprError):
        d.e.group_add_source(d.gid, ranked[16])
    with pytest.raises(eng.DpprError):
        d.e.group_remove_source(one, 0)
    assert eng.live_bytes() == mem and d.e.group_sources(one) == ranked[:1]
    d.check("refused")
    d.e.group_remove_source(d.gid, 15)   # (both are accepted the other way round)
    assert d.e.group_add_source(one, ranked[1])[0] == 1
    d.close()


def test_add_then_remove_gives_the_memory_back():
    gc.collect()  # (engines other tests dropped without closing them)
    base = eng.live_bytes()
    V, e1, e2 = small_stream()
    ranked = ranked_sources(V, e1, e2, SMALL["W"], 0)
    d = Driver(V, e1, e2, directed=0, sources=ranked[:10], **SMALL)
    d.batches(1)

    def pair():
        d.churn("add", source=ranked[16])          # rows of 80 -> 96 bytes
        check_group(d.e, d.gid, 11, ks=(10,), min_ps=(0.0,))
        d.e.group_read_at(d.gid, ranked[:4])
        d.churn("remove", 10)
        check_group(d.e, d.gid, 10, ks=(10,), min_ps=(0.0,))

    pair()  # warm: every lazily allocated buffer exists afterwards
    warm = eng.live_bytes()
    assert warm[0] > base[0]
    pair()
    assert eng.live_bytes() == warm
    d.churn("add", source=ranked[16])
    assert eng.live_bytes()[0] > warm[0]  # two more doubles per row in p and r
    d.churn("remove", 10)
    assert eng.live_bytes() == warm
    d.batches(1)
    d.close()
    assert eng.live_bytes() == base
