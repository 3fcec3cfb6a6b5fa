"""Every sweep and push form, both schedules, source groups, the merged loop, renumbering and overlapped slides against the
oracle BIT FOR BIT, on conflict-free layered streams (tests/cf_stream.py; premises checked by
tests/test_conflict_free_streams.py).

On these directed streams a row receives at most one nonzero term per sweep and no vertex shares a frontier with its
parent, so the only freedom the atomic sums have (their arrival order) is gone: p and r must be the oracle's to the
last bit after the from-scratch solve and after every batch, whatever the launch form. A kernel that computes
(1 - a) x / den with a different rounding (push_term without its correction step, (1 - a) (x / den), FMA contraction),
or repairs as (r - x) + t, fails here while the tolerance of test_engine_gpu.py lets it pass. Undirected streams are
out of scope: every edge runs both ways, so there is no dead set and no single-term row.

Streams on which a vertex and its parent DO share frontiers (`parents_in_frontier`) keep one term per row: there the
gather forms, which repair in the fixed order (r + t) - x, are held to schedule C bit for bit as well.
"""
import functools
import threading

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests.cf_stream import conflict_free_stream
from tests.test_conflict_free_streams import EPS, SMALL, same
from tests.test_engine_gpu import MERGE_IDS, MERGE_TUNINGS, TUNING_IDS, TUNINGS, VARIANT_IDS, VARIANT_TUNINGS

pytestmark = pytest.mark.gpu

W, C, BATCHES = SMALL["W"], SMALL["c"], SMALL["batches"]


@functools.lru_cache(maxsize=None)
def stream(seed=1, **kw):
    return conflict_free_stream(seed=seed, **dict(SMALL, **kw))


def advance(g, e):
    assert not g.stream_updates()
    g.inc_construct(1)
    e.set_batch(*g.batch())
    e.slide(*g.new_stream())


def assert_bits(p, r, s, what):
    assert same(p, s.p), ("p", what, int(np.sum(p != s.p)), float(np.max(np.abs(p - s.p))))
    assert same(r, s.r), ("r", what, int(np.sum(r != s.r)), float(np.max(np.abs(r - s.r))))


def assert_form_ran(tuning, st):
    """The launch form a tuning names ran (no vacuous passes)."""
    pmf = tuning.get("pull_min_frontier", 0)
    assert st["iterations"] > 0
    if pmf == -1:                                     # every iteration a push (push_launches counts only when profiling)
        assert st["pull_iterations"] == 0, st
    elif pmf == 1:
        assert st["pull_iterations"] == st["iterations"], st
    elif pmf > 1:
        assert 0 < st["pull_iterations"] < st["iterations"], st
    if "binned" in tuning:
        assert st["binned_sweeps"] == st["pull_iterations"] > 0, st
    else:
        assert st["binned_sweeps"] == 0, st
    if tuning.get("persistent") == 0:
        assert st["persist_launches"] == 0, st
    elif tuning.get("persist_timeout_us") == -1:
        assert st["persist_aborts"] > 0, st
    elif pmf == 1 and not tuning.get("sweep_bitmap"):  # resident sweeps (the bitmap is a per-iteration form)
        assert st["persist_launches"] > 0 and st["persist_aborts"] == 0, st


def run_slot(tuning, schedule, init, inc, trace=False, strm=None, source_index=2, batches=BATCHES):
    """One slot against one oracle state (init / inc: the oracle's from-scratch and per-batch schedule)."""
    V, e1, e2, meta = strm or stream()
    src = int(meta["sources"][source_index])
    g = orc.Graph(V, e1, e2, 1, W, C)
    s = orc.State(V, src, EPS)
    e = eng.Engine(V, W, 1, C, schedule=schedule, **tuning)
    e.load_window(*g.window_edges())
    slot = e.add_source(src)
    for k in range(batches + 1):
        if trace:
            s.trace(True)
            e.trace_enable(slot, True)
        if k:
            advance(g, e)
            inc(s, g)
            e.update(slot, EPS)
        else:
            init(s, g)
            e.init_solve(slot, EPS)
        p, r = e.read(slot)
        assert_bits(p, r, s, k)
        if trace:
            want, got = s.traced_frontiers(), e.trace_get(slot)
            assert len(got) == len(want) and len(want) > 2, k
            for a, b in zip(got, want):
                assert np.array_equal(np.sort(a), np.sort(b)), k
    st, want = e.stats(slot), s.stats()
    assert (st["iterations"], st["sum_F"], st["sum_E"]) == (want["iters"], want["F"], want["E"])
    e.close()
    return st


SYNC_C = (lambda s, g: s.sync_execute(g), lambda s, g: s.sync_inc_execute(g))
CILK_A = (lambda s, g: s.cilk_execute(g), lambda s, g: s.cilk_inc_execute(g))


# ------------------------------------------------------------------ single source
@pytest.mark.parametrize("tuning", TUNINGS, ids=TUNING_IDS)
def test_sync_schedule_bit_exact(tuning):
    assert_form_ran(tuning, run_slot(tuning, eng.SCHEDULE_SYNC, *SYNC_C))


@pytest.mark.parametrize("tuning", TUNINGS, ids=TUNING_IDS)
def test_sync_schedule_traced_frontiers_bit_exact(tuning):
    """With the trace on (one launch per iteration): every frontier set, and p / r bit for bit."""
    run_slot(tuning, eng.SCHEDULE_SYNC, *SYNC_C, trace=True)


@pytest.mark.parametrize("tuning", TUNINGS, ids=TUNING_IDS)
def test_eager_schedule_bit_exact_with_schedule_a(tuning):
    """The north-star comparison (cpu/PPRCPUMTCilkRev at -t 1) is bitwise on these streams."""
    assert_form_ran(tuning, run_slot(tuning, eng.SCHEDULE_EAGER, *CILK_A))


@pytest.mark.parametrize("tuning", VARIANT_TUNINGS, ids=VARIANT_IDS)
@pytest.mark.parametrize("variant", [1, 3])
def test_variants_bit_exact(variant, tuning):
    run_slot(dict(tuning, variant=variant), eng.SCHEDULE_SYNC, lambda s, g: s.variant_execute(g, variant),
             lambda s, g: s.variant_inc_execute(g, variant), trace=True)


@pytest.mark.parametrize("tuning", MERGE_TUNINGS, ids=MERGE_IDS)
def test_merged_loop_single_source_bit_exact(tuning):
    div = 4
    V, e1, e2, meta = stream()
    src = int(meta["sources"][2])
    g = orc.Graph(V, e1, e2, 1, W, C)
    m = orc.State(V, src, EPS)
    e = eng.Engine(V, W, 1, C, **dict(tuning, merge_phases=div))
    e.load_window(*g.window_edges())
    slot = e.add_source(src)
    m.cilk_execute(g)
    e.init_solve(slot, EPS)
    assert_bits(*e.read(slot), m, 0)
    for k in range(1, BATCHES + 1):
        advance(g, e)
        m.merged_inc_execute(g, EPS / div)
        e.update(slot, EPS)
        assert_bits(*e.read(slot), m, k)
    st = e.stats(slot)
    if tuning.get("pull_min_frontier") == -1:
        assert st["pull_iterations"] == 0 and st["iterations"] > 0
    else:
        assert st["pull_iterations"] > 0 and (st["binned_sweeps"] > 0) == ("binned" in tuning)
    e.close()


# ------------------------------------------------------------------ source groups
def run_group(sources, seeding="tails", tuning=None, resident=True, push=None, div=0, batches=BATCHES, reads=None):
    """A source group against one oracle state per source: schedule C, or the merged loop at eps / div. `reads`: a list that
    takes every (p, r) read, in order."""
    V, e1, e2, meta = stream()
    tuning = dict(tuning or {}, **(dict(merge_phases=div) if div else {}))
    e = eng.Engine(V, W, 1, C, **tuning)
    e.set_group_seeding(seeding == "tails")
    e.set_group_resident(resident)
    if push is not None:
        e.set_group_push(*push)
    g = orc.Graph(V, e1, e2, 1, W, C)
    states = [orc.State(V, s, EPS) for s in sources]
    e.load_window(*g.window_edges())
    gid = e.add_source_group(sources)
    for s in states:
        s.sync_execute(g)
    e.group_init_solve(gid, EPS)
    for k in range(batches + 1):
        if k:
            advance(g, e)
            for s in states:
                if div:
                    s.merged_inc_execute(g, EPS / div)
                else:
                    s.sync_inc_execute(g)
            e.group_update(gid, EPS)
        for i, s in enumerate(states):
            p, r = e.group_read(gid, i)
            assert_bits(p, r, s, (k, i))
            if reads is not None:
                reads.append((p.copy(), r.copy()))
    st = e.group_stats(gid)
    assert st["sum_F"] == sum(s.stats()["F"] for s in states) and st["sum_E"] == sum(s.stats()["E"] for s in states)
    e.close()
    return st


def group_sources(n):
    return [int(x) for x in stream()[3]["sources"][:n]]


@pytest.mark.parametrize("seeding", ["tails", "dense"])
@pytest.mark.parametrize("nsrc", list(range(1, 17)))
def test_source_group_every_width(nsrc, seeding):
    """Widths 2..16 cover every row width gw, with and without padding lanes."""
    st = run_group(group_sources(nsrc), seeding)
    assert st["pull_iterations"] > 0


@pytest.mark.parametrize("mode", ["one-launch-per-sweep", "multi-sweep", "multi-sweep-3-at-a-time", "rollcall-fails"])
@pytest.mark.parametrize("nsrc", [4, 10, 11, 12])
def test_source_group_launch_forms(nsrc, mode):
    tuning = {"multi-sweep-3-at-a-time": dict(chunk_iters=3), "rollcall-fails": dict(persist_timeout_us=-1)}.get(mode)
    st = run_group(group_sources(nsrc), tuning=tuning, resident=mode != "one-launch-per-sweep")
    if mode == "one-launch-per-sweep":
        assert st["persist_launches"] == 0 and st["pull_iterations"] > 0
    elif mode == "rollcall-fails":
        assert st["persist_launches"] >= 1 and st["persist_aborts"] >= 1
    else:
        assert st["persist_launches"] > 0 and st["persist_aborts"] == 0


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "one-sweep"])
@pytest.mark.parametrize("nsrc", [3, 10])
def test_source_group_independent_of_chunking(nsrc, resident):
    """How a loop is cut into chunks (dppr_set_tuning chunk_iters; dppr_loop_plan.hpp sizes every chunk and launch from it and from
    the loop histories) changes what is launched and nothing else: after a solve and after each of three updates the bits of p and r
    and (iterations, sum_F, sum_E) are the same for 1, 2, 5 and 24 sweeps per chunk. One sweep per chunk without residency is the
    smallest shape at which an off-by-one in a chunk size or in a history changes the launches; ten sources run SPL = 2, NVX = 512."""
    want = None
    for chunk in (1, 2, 5, 24):
        reads = []
        st = run_group(group_sources(nsrc), tuning=dict(chunk_iters=chunk, schedule=eng.SCHEDULE_SYNC), resident=resident, batches=3, reads=reads)
        assert (st["persist_launches"] > 0) == (resident and chunk > 1), (chunk, st)
        got = (reads, (st["iterations"], st["sum_F"], st["sum_E"]))
        if want is None:
            want = got
            continue
        assert got[1] == want[1], (chunk, got[1], want[1])
        assert len(reads) == len(want[0]) == 4 * nsrc
        for (p, r), (wp, wr) in zip(reads, want[0]):
            assert same(p, wp) and same(r, wr), chunk


GPUSH_MODES = {"automatic": (-1, 0), "never": (0, 0), "as-early-as-possible": (10**9, 0), "as-early-as-possible-chunk2": (10**9, 0),
               "tiny-lists": (10**9, 1024), "below-50-pairs": (50, 0), "iterations-call-themselves-off": (10**9, 0, 3000)}


@pytest.mark.parametrize("mode", list(GPUSH_MODES))
@pytest.mark.parametrize("nsrc", [3, 10, 16])
def test_source_group_tail_as_pushes(nsrc, mode):
    """The group push tail (dppr_gpush.hpp): k_gpush_snap zeroes at the snapshot, which equals C's (r + 0) - x here."""
    tuning = dict(chunk_iters=2) if mode.endswith("chunk2") or mode.endswith("off") else None
    st = run_group(group_sources(nsrc), tuning=tuning, resident=False, push=GPUSH_MODES[mode])
    assert st["persist_launches"] == 0
    if mode == "never":
        assert st["pull_iterations"] == st["iterations"]
    elif mode != "tiny-lists":
        assert st["pull_iterations"] < st["iterations"]


@pytest.mark.parametrize("mode", ["sweeps", "push-tail", "multi-sweep"])
@pytest.mark.parametrize("nsrc", [3, 10, 16])
def test_merged_loop_source_group_bit_exact(nsrc, mode):
    tuning = dict(chunk_iters=3) if mode == "multi-sweep" else None
    push = (40, 0, 0) if mode == "push-tail" else (0, 0, 0)
    st = run_group(group_sources(nsrc), tuning=tuning, resident=mode == "multi-sweep", push=push, div=4)
    if mode == "push-tail":
        assert st["pull_iterations"] < st["iterations"]
    elif mode == "multi-sweep":
        assert st["persist_launches"] > 0


# ------------------------------------------------------------------ renumbering, overlapped slides
RENUMBER = dict(V=1 << 13, levels=6, W=12000, c=500, batches=16, fan_max=1000, dup_frac=0.05)




@pytest.mark.parametrize("mode", ["slot", "group"])
def test_renumbered_id_space_bit_exact(mode):
    V, e1, e2, meta = conflict_free_stream(seed=5, churn=True, **RENUMBER)
    Wr, Cr, batches = RENUMBER["W"], RENUMBER["c"], RENUMBER["batches"]
    sources = [int(x) for x in meta["sources"][:(5 if mode == "group" else 1)]]
    g = orc.Graph(V, e1, e2, 1, Wr, Cr)
    e = eng.Engine(V, Wr, 1, Cr, schedule=eng.SCHEDULE_SYNC)
    e.set_renumbering(1, growth_pct=10, min_parked=16)
    e.load_window(*g.window_edges())
    h = e.add_source_group(sources) if mode == "group" else e.add_source(sources[0])
    states = [orc.State(V, s, EPS) for s in sources]
    for s in states:
        s.sync_execute(g)
    (e.group_init_solve if mode == "group" else e.init_solve)(h, EPS)
    for k in range(batches + 1):
        if k:
            advance(g, e)
            for s in states:
                s.sync_inc_execute(g)
            (e.group_update if mode == "group" else e.update)(h, EPS)
        for i, s in enumerate(states):
            assert_bits(*(e.group_read(h, i) if mode == "group" else e.read(h)), s, (k, i))
    ids = e.id_space()
    assert ids["parked"] > 0 and ids["renumberings"] > 0, ids
    e.close()


@pytest.mark.parametrize("mode", ["slot", "group"])
def test_overlapped_slides_bit_exact(mode):
    """dppr_slide_concurrent builds batch k + 1's epoch on another thread while batch k is solved (n_epochs = 2)."""
    V, e1, e2, meta = stream()
    sources = [int(x) for x in meta["sources"][:(10 if mode == "group" else 1)]]
    pre = orc.Graph(V, e1, e2, 1, W, C)
    stage = []
    for _ in range(BATCHES):
        assert not pre.stream_updates()
        pre.inc_construct(1)
        stage.append(([x.copy() for x in pre.batch()], [x.copy() for x in pre.new_stream()]))
    g = orc.Graph(V, e1, e2, 1, W, C)
    e = eng.Engine(V, W, 1, C, n_epochs=2, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    h = e.add_source_group(sources) if mode == "group" else e.add_source(sources[0])
    states = [orc.State(V, s, EPS) for s in sources]
    for s in states:
        s.sync_execute(g)
    (e.group_init_solve if mode == "group" else e.init_solve)(h, EPS)

    def build(k, concurrent, box):
        e.set_batch(*stage[k - 1][0])
        box.append(e.slide(*stage[k - 1][1], concurrent=concurrent))

    box = []
    build(1, False, box)
    epoch, beside = box[0], 0
    for k in range(1, BATCHES + 1):
        th, box = None, []
        if k < BATCHES:
            th = threading.Thread(target=build, args=(k + 1, True, box))
            th.start()
        (e.group_update if mode == "group" else e.update)(h, EPS, epoch=epoch)
        assert not g.stream_updates()
        g.inc_construct(1)
        for i, s in enumerate(states):
            s.sync_inc_execute(g)
            assert_bits(*(e.group_read(h, i) if mode == "group" else e.read(h)), s, (k, i))
        if th is not None:
            th.join()
            beside += 1
            epoch = box[0]
    assert beside == BATCHES - 1
    e.close()


# ------------------------------------------------------------------ gather forms with a vertex and its parent in one frontier
GATHER_TUNINGS = [dict(pull_min_frontier=1, persistent=0), dict(pull_min_frontier=1, persistent=0, pull_block=256, big_row_edges=8),
                  dict(pull_min_frontier=1), dict(pull_min_frontier=1, persistent=0, binned=(2, 1, 1, 64, 0, 64, 64))]
GATHER_IDS = ["pull-no-persist", "pull-wg256-bigrows", "pull-resident", "binned-tiny-blocks"]


@pytest.mark.parametrize("tuning", GATHER_TUNINGS, ids=GATHER_IDS)
def test_gather_sweeps_repair_as_r_plus_t_minus_x(tuning):
    """Streams whose batches mix both level parities: a vertex and its parent share frontiers, and a frontier row gathers
    its parent's term. Every row still receives one term, and the gather forms repair in the fixed order (r + t) - x of
    schedule C: bit for bit."""
    strm = stream(4, parents_in_frontier=True)
    assert_form_ran(tuning, run_slot(tuning, eng.SCHEDULE_SYNC, *SYNC_C, strm=strm))


# ------------------------------------------------------------------ one large stream
LARGE = dict(V=1 << 22, levels=6, W=4_000_000, c=200_000, batches=3, fan_max=100_000, dup_frac=0.02, live_frac=0.3)


@functools.lru_cache(maxsize=None)
def large_stream():
    return conflict_free_stream(seed=9, **LARGE)


@pytest.mark.parametrize("form", ["default", "binned-forced"])
def test_large_stream_slot_and_ten_source_group(form):
    """V = 2^22, a window of 4 M edges, fan rows above 2^16 edges (den > 65 536): one slot and one 10-source group (the
    headline's k_gsweep shape), default tunings; 'binned-forced' forces the slot onto binned sweeps (every iteration a
    sweep, dppr_set_binned_sweep mode 2, no resident launches), which the defaults do not pick on this window by themselves."""
    V, e1, e2, meta = large_stream()
    Wl, Cl = LARGE["W"], LARGE["c"]
    deg = np.bincount(e1[:Wl], minlength=V)
    assert deg.max() > 1 << 16
    tuning = dict(pull_min_frontier=1, persistent=0, binned=2) if form == "binned-forced" else {}
    g = orc.Graph(V, e1, e2, 1, Wl, Cl)
    e = eng.Engine(V, Wl, 1, Cl, schedule=eng.SCHEDULE_SYNC, **tuning)
    e.load_window(*g.window_edges())
    sources = [int(x) for x in meta["sources"][:10]]
    slot = e.add_source(sources[0])
    gid = e.add_source_group(sources)
    single = orc.State(V, sources[0], EPS)
    states = [orc.State(V, s, EPS) for s in sources]
    for s in [single] + states:
        s.sync_execute(g)
    e.init_solve(slot, EPS)
    e.group_init_solve(gid, EPS)
    for k in range(LARGE["batches"] + 1):
        if k:
            advance(g, e)
            for s in [single] + states:
                s.sync_inc_execute(g)
            e.update(slot, EPS)
            e.group_update(gid, EPS)
        assert_bits(*e.read(slot), single, ("slot", k))
        for i, s in enumerate(states):
            assert_bits(*e.group_read(gid, i), s, (k, i))
    st, gst = e.stats(slot), e.group_stats(gid)
    assert (st["iterations"], st["sum_F"], st["sum_E"]) == tuple(single.stats()[x] for x in ("iters", "F", "E"))
    assert gst["sum_F"] == sum(s.stats()["F"] for s in states) and gst["sum_E"] == sum(s.stats()["E"] for s in states)
    assert gst["pull_iterations"] > 0
    if form == "binned-forced":
        assert st["binned_sweeps"] == st["pull_iterations"] == st["iterations"] > 0, st
    e.close()
