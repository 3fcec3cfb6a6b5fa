"""Nothing leaks: every device and pinned-host allocation of an engine is owned by a buffer that goes with its owner
(csrc/dppr_devbuf.hpp), so after Engine.close() the library's own count of live bytes (dppr_debug_live_bytes: process-wide, blind
to the device's other tenants) is back where it was before the engine was created -- whichever of the allocate-on-first-use and
grow-on-demand buffers the scenario touched. Each scenario carries a witness that the path it is about really ran.
Correctness of the results is the business of the other suites; small windows, no oracle here."""
import gc
import threading

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from dynamicppr_amd.stream import SlidingStream, Workload
from tests.test_renumbering_gpu import churn_stream

pytestmark = pytest.mark.gpu
EPS = 1e-9


@pytest.fixture
def baseline():
    """The counters before the scenario (engines that earlier tests left to the garbage collector are gone first); checked again
    after it."""
    gc.collect()
    before = eng.live_bytes()
    yield before
    gc.collect()
    assert eng.live_bytes() == before, f"live (device, pinned) bytes {eng.live_bytes()} after the scenario, {before} before it"


class Run:
    """An engine over a sliding window of a stream, driven without the oracle."""

    def __init__(self, V, e1, e2, W, c, directed, **tuning):
        self.stream = SlidingStream(V, e1, e2, directed, Workload(W, c, 0, 0))
        self.e = eng.Engine(V, W, directed, c, **tuning)
        self.e.load_window(*self.stream.serialize_edge_stream())

    def slide(self, concurrent=False):
        assert not self.stream.stream_updates()
        self.e.set_batch(*self.stream.batch_arrays())
        return self.e.slide(*self.stream.new_arrays(), concurrent=concurrent)


def alive(before):
    dev, pin = eng.live_bytes()
    assert dev > before[0] and pin > before[1], "an engine holds device and pinned memory while it is alive"
    return dev, pin


@pytest.mark.parametrize("nsrc", [10, 16])
def test_group_whose_push_tail_ran(baseline, nsrc):
    """Group::plist / ppre / pctl are allocated by the first push tail of a group's loop."""
    V, e1, e2 = datagen.rmat_stream(13, 70000, 21)
    W, c, directed = 20000, 200, 1
    run = Run(V, e1, e2, W, c, directed)
    run.e.set_group_resident(False)
    run.e.set_group_push(10**9, 0, 0)  # (the push form as early as possible)
    gid = run.e.add_source_group([int(x) for x in datagen.top_sources(V, e1, e2, W, directed, nsrc)])
    before_tail = alive(baseline)
    run.e.group_init_solve(gid, EPS)
    for _ in range(4):
        run.slide()
        run.e.group_update(gid, EPS)
    st = run.e.group_stats(gid)
    assert st["pull_iterations"] < st["iterations"], "no iteration ran as pushes: the scenario did not reach the push tail"
    assert alive(baseline)[0] > before_tail[0]  # (the lists are there)
    run.e.close()


@pytest.mark.parametrize("form", ["threshold", "fast-frontier", "eager-status", "vanilla-status", "merged-loop"])
def test_single_source_under_every_duplicate_filter(baseline, form):
    """The reference's variants 0-3 and the merged loop: variants 2 / 3 and the merged loop filter duplicates through Slot::status,
    allocated by the first loop that wants it (push iterations only here: nothing else is allocated on the way)."""
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    W, c, directed = 600, 20, 1
    variant = {"threshold": 0, "fast-frontier": 1, "eager-status": 2, "vanilla-status": 3, "merged-loop": 0}[form]
    run = Run(V, e1, e2, W, c, directed, variant=variant, merge_phases=(True if form == "merged-loop" else None), pull_min_frontier=-1,
              persistent=0)
    slot = run.e.add_source(int(datagen.top_sources(V, e1, e2, W, directed, 1)[0]))
    before_solve = alive(baseline)
    run.e.init_solve(slot, EPS)
    for _ in range(5):
        run.slide()
        run.e.update(slot, EPS)
    if form in ("eager-status", "vanilla-status", "merged-loop"):  # (the merged loop is the update's: the from-scratch solve has one sign)
        assert alive(baseline)[0] >= before_solve[0] + 4 * V, "no status array (one int per vertex) was allocated"
    run.e.close()


def test_topk_and_point_queries(baseline):
    """The first query allocates the top-k work space (device and pinned), the id map's device copy, the candidate lists and the
    point-read buffer; a larger read grows the latter."""
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    W, c, directed = 600, 20, 0
    run = Run(V, e1, e2, W, c, directed)
    top = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 5)]
    slot, gid = run.e.add_source(top[0]), run.e.add_source_group(top)
    run.e.init_solve(slot, EPS)
    run.e.group_init_solve(gid, EPS)
    before_queries = alive(baseline)
    ids, p, _ = run.e.topk(slot, 10)
    assert len(ids) == 10 and p[0] > 0
    run.e.group_topk(gid, 50)
    run.e.read_at(slot, top[:2])
    run.e.group_read_at(gid, np.arange(V, dtype=np.int32))
    after = alive(baseline)
    assert after[0] > before_queries[0] and after[1] > before_queries[1]
    run.e.close()


@pytest.mark.parametrize("oom", [False, True])
def test_binned_tables(baseline, monkeypatch, oom):
    """A window that sweeps binned: engine-level scratch plus per-epoch tables -- all of them, or (DPPR_TEST_BIN_OOM: every one of
    their allocations reports out-of-memory) none, the calls succeeding either way."""
    if oom:
        monkeypatch.setenv("DPPR_TEST_BIN_OOM", "1")
    V, e1, e2 = datagen.rmat_stream(12, 60000, 5)
    W, c, directed = 20000, 200, 1
    run = Run(V, e1, e2, W, c, directed, binned=(2, 0, 0, 0, 0), pull_min_frontier=1, persistent=0)
    slot = run.e.add_source(int(datagen.top_sources(V, e1, e2, W, directed, 1)[0]))
    run.e.init_solve(slot, EPS)
    for _ in range(3):
        run.slide()
        run.e.update(slot, EPS)
    assert (run.e.bin_tables(arrays=False) is None) == oom
    alive(baseline)
    run.e.close()


def test_renumbering_and_revivals(baseline):
    """A stream that churns through the id range: renumberings (function-local scratch) and revived vertices whose rows move
    (the mv_* scratch, grown on demand), for a slot and a group."""
    V, W, c, batches, directed = 4096, 1500, 100, 60, 1
    e1, e2 = churn_stream(V, W + batches * c, 400, 6)
    run = Run(V, e1, e2, W, c, directed, schedule=eng.SCHEDULE_SYNC)
    run.e.set_renumbering(1, growth_pct=10, min_parked=16)
    slot, gid = run.e.add_source(0), run.e.add_source_group([0, 1, int(e1[0]), 2, 3])
    run.e.init_solve(slot, EPS)
    run.e.group_init_solve(gid, EPS)
    for _ in range(batches):
        run.slide()
        run.e.update(slot, EPS)
        run.e.group_update(gid, EPS)
    ids = run.e.id_space()
    assert ids["renumberings"] >= 1 and ids["revivals"] >= 1, ids
    alive(baseline)
    run.e.close()


def test_slide_concurrent_beside_a_solve(baseline):
    """The builder thread builds epoch k + 1 (its own stream and scratch) while the solver thread updates on epoch k."""
    V, W, c, batches, directed = 4096, 600, 60, 20, 1
    e1, e2 = churn_stream(V, W + (batches + 1) * c, 400, 5)
    stream = SlidingStream(V, e1, e2, directed, Workload(W, c, 0, 0))
    e = eng.Engine(V, W, directed, c, n_epochs=2, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*stream.serialize_edge_stream())
    slot = e.add_source(0)
    e.init_solve(slot, EPS)

    def build(concurrent, box):
        assert not stream.stream_updates()
        e.set_batch(*stream.batch_arrays())
        box.append(e.slide(*stream.new_arrays(), concurrent=concurrent))

    box = []
    build(False, box)
    beside = 0
    for k in range(1, batches + 1):
        epoch, box, th = box[0], [], None
        if not e.renumbering_due():
            th = threading.Thread(target=build, args=(True, box))
            th.start()
        e.update(slot, EPS, epoch=epoch)
        if th is not None:
            th.join()
            beside += 1
        else:
            build(False, box)
    assert beside >= batches // 2
    alive(baseline)
    e.close()


@pytest.mark.parametrize("first", [0, 1])
def test_two_engines_destroyed_in_either_order(baseline, first):
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    W, c, directed = 600, 20, 1
    src = int(datagen.top_sources(V, e1, e2, W, directed, 1)[0])
    runs = [Run(V, e1, e2, W, c, directed), Run(V, e1, e2, W, c, directed, pull_min_frontier=1, persistent=0)]
    slots = [r.e.add_source(src) for r in runs]
    for r, s in zip(runs, slots):
        r.e.init_solve(s, EPS)
    both = alive(baseline)
    runs[first].e.close()
    one = alive(baseline)
    assert one[0] < both[0] and one[1] < both[1]
    other = runs[1 - first]
    other.slide()
    other.e.update(slots[1 - first], EPS)  # (the survivor is untouched)
    p, r = other.e.read(slots[1 - first])
    assert p[src] > 0 and np.max(np.abs(r)) <= EPS
    other.e.close()


def test_steady_stream_settles(baseline):
    """The grow-on-demand buffers settle: over a stream that repeats itself, once one whole period has gone through the window the
    engine's device memory does not grow over 50 further batches (a slot and a group, default launch forms)."""
    V, a, b = datagen.rmat_stream(9, 6000, 11)
    W, c, directed = 600, 30, 1
    period = len(a) // c
    e1, e2 = np.tile(a[:period * c], 3), np.tile(b[:period * c], 3)
    run = Run(V, e1, e2, W, c, directed)
    top = [int(x) for x in datagen.top_sources(V, a, b, W, directed, 3)]
    slot, gid = run.e.add_source(top[0]), run.e.add_source_group(top)
    run.e.init_solve(slot, EPS)
    run.e.group_init_solve(gid, EPS)

    def batches(n):
        for _ in range(n):
            run.slide()
            run.e.update(slot, EPS)
            run.e.group_update(gid, EPS)

    batches(period)
    settled = alive(baseline)
    batches(50)
    now = alive(baseline)
    assert now[0] <= settled[0] and now[1] <= settled[1], f"(device, pinned) bytes grew from {settled} to {now} over 50 steady batches"
    run.e.close()
