"""The one scratch state of the weighted, changes and ranked queries (QueryWork::Scratch): calls of the three families that follow
each other on one engine give, bit for bit, what each gives on an engine that has made only that call; a family that comes
second finds the scratch of the first and allocates none of its own; the point reads report their device time. Ids are compared
with array_equal, doubles by their uint64 patterns."""
import gc

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_renumbering_gpu import churn_stream
from tests.test_weighted_gpu import EPS, bits
from tests.util import small_stream

pytestmark = pytest.mark.gpu

NARROW, WIDE = 2, 10
ALL = eng.EXCLUDE_SEEDS | eng.EXCLUDE_IN_NEIGHBOURS | eng.EXCLUDE_OUT_NEIGHBOURS
K = 50


class Built:
    """An engine with a slot and groups of width 2 and 10, solved, marked, and two batches on. plain: the small R-MAT window of
    tests/test_rank_gpu.py; parked: the churn stream of its test_id_space_parked_and_unnamed_vertices, renumbered at slide time,
    marked two batches before the end."""

    def __init__(self, parked):
        if parked:
            V, W, c, batches, mark_at = 4096, 1500, 100, 60, 58
            e1, e2 = churn_stream(V, W + batches * c, 400, 5)
            srcs = list(range(WIDE))
        else:
            V, e1, e2 = small_stream()
            W, c, batches, mark_at = 600, 20, 2, 0
            srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, 1, WIDE)]
        g = orc.Graph(V, e1, e2, 1, W, c)
        e = self.e = eng.Engine(V, W, 1, c)
        if parked:
            e.set_renumbering(1, growth_pct=10, min_parked=16)
        e.load_window(*g.window_edges())
        self.V = V
        self.slot = e.add_source(srcs[0])
        self.narrow, self.wide = e.add_source_group(srcs[:NARROW]), e.add_source_group(srcs)
        e.init_solve(self.slot, EPS)
        for gid in (self.narrow, self.wide):
            e.group_init_solve(gid, EPS)
        for b in range(batches + 1):
            if b == mark_at:
                e.mark(self.slot)
                e.group_mark(self.narrow)
                e.group_mark(self.wide)
            if b == batches:
                break
            assert not g.stream_updates()
            g.inc_construct(1)
            e.set_batch(*g.batch())
            e.slide(*g.new_stream())
            e.update(self.slot, EPS)
            for gid in (self.narrow, self.wide):
                e.group_update(gid, EPS)
        sp = e.id_space()
        self.rows = sp["ids"] + sp["parked"]
        assert self.rows % 128 != 0 and self.rows > 128, sp       # (more than one tile, the last one short)
        assert sp["parked"] > 0 or not parked, sp


def calls():
    """The sequence of the interleaving test: (name, the call on a Built, the call as an engine makes it alone). The two differ in
    the re-marking call only: alone it leaves the mark as it is, so that the sequence after it finds the same mark and state --
    the results of a call do not depend on `remark`, which the comparison then holds too."""
    rng = np.random.default_rng(5)
    w16 = rng.standard_normal((16, WIDE))
    w1 = rng.random((1, WIDE))
    deg_all = eng.Engine.rank_spec(eng.FACTOR_DEG, exclude=ALL)
    seq = [("weighted q=16, wide", lambda b: b.e.group_topk_weighted(b.wide, w16, K)),
           ("changes, slot", lambda b: [b.e.changes(b.slot, K)]),
           ("ranked DEG + all exclusions, wide", lambda b: b.e.group_topk_ranked(b.wide, K, 0.0, deg_all)),
           ("changes with remark, narrow", lambda b: b.e.group_changes(b.narrow, K, 0.0, True)),
           ("weighted q=1, wide", lambda b: b.e.group_topk_weighted(b.wide, w1, K)),
           ("ranked, slot", lambda b: [b.e.topk_ranked(b.slot, K)]),
           ("changes, wide", lambda b: b.e.group_changes(b.wide, K))]
    return [(name, call, (lambda b: b.e.group_changes(b.narrow, K)) if "remark" in name else call) for name, call in seq]


def same(got, want, what):
    """Two results of one call: lists of tuples of arrays (ids, doubles ..) and, for changes, the moved count."""
    assert len(got) == len(want) and len(got) > 0, what
    for lane, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (what, lane)
        for x, y in zip(a, b):
            if isinstance(x, np.ndarray) and x.dtype == np.float64:
                assert np.array_equal(bits(x), bits(y)), (what, lane)
            else:
                assert np.array_equal(x, y), (what, lane)


@pytest.mark.parametrize("parked", [False, True], ids=["plain", "parked"])
def test_interleaved_calls_equal_calls_alone(parked):
    """Two engines built alike do not reach bit-equal states (the solves add with atomics), and a group's state cannot be written.
    So the engine that makes only the call and the engine that runs the sequence are one engine per call of the sequence: the call
    alone first, on an engine that has made no other query, then the whole sequence, whose result at that position must repeat it."""
    seq = calls()
    for i, (name, _, alone) in enumerate(seq):
        b = Built(parked)
        want = alone(b)
        got = [call(b) for _, call, _ in seq][i]
        again = b.e.group_changes(b.narrow, K)
        b.e.close()
        assert any(len(lane[0]) > 0 for lane in want), name       # (the call has something to say)
        same(got, want, name)
        assert all(len(ids) == 0 and moved == 0 for ids, _, _, moved in again), name   # (the sequence's re-mark took place)


def test_the_families_share_one_scratch():
    gc.collect()
    before = eng.live_bytes()
    b = Built(False)
    b.e.group_changes(b.wide, K)
    held = eng.live_bytes()
    assert held[0] > before[0]
    b.e.group_topk_ranked(b.wide, K)      # (NULL spec: no marking stage; the scores go where |d| went)
    assert eng.live_bytes() == held
    b.e.close()
    assert eng.live_bytes() == before


@pytest.mark.parametrize("which", ["read_at", "group_score_at"])
def test_point_reads_report_their_device_time(which):
    b = Built(False)
    b.e.set_profiling(1)
    assert b.e.query_ms() < 0                # (nothing has been timed on this engine yet)
    ids = np.arange(0, b.V, 3, dtype=np.int32)
    if which == "read_at":
        b.e.read_at(b.slot, ids)
    else:
        b.e.group_score_at(b.wide, np.ones((3, WIDE)), ids)
    assert b.e.query_ms() > 0
    b.e.close()
