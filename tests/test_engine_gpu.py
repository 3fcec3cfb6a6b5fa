"""GPU parity tests: the HIP engine (through the C ABI) against the CPU oracle.

Bars (DESIGN.md "Parity"):
  * integer / index work (CSR, out-degrees, Inspect frontier, per-iteration frontier
    sets in the synchronous schedule): BIT-EXACT;
  * the incremental residual fix-up (IncrementalBatchUpdate): BIT-EXACT doubles;
  * p / r after a solve: synchronous schedule within SYNC_TOL of the oracle's
    synchronous schedule (only the order of the atomic sums differs), eager schedule
    within the north-star tolerance 1e-9 of cpu/PPRCPUMTCilkRev (-t 1 restatement),
    plus the reference's own Validate() criteria (|r| < eps, |p - p_pow| < 100 eps).
"""
import sys
import time

import threading

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.util import (Scenario, golden_names, invariant_max_err_np, load_golden, sorted_csr,
                        window_directed_edges)

pytestmark = pytest.mark.gpu

NORTH_STAR_TOL = 1e-9   # BASELINE.json: "within the repo's 1e-9 tolerance"
SYNC_TOL = 1e-14        # same schedule, only float-atomic arrival order differs (ulps of values <= 1, ~100 iterations);
                        # where that order is fixed (one term per row) tests/test_conflict_free_gpu.py holds p / r bit for bit
INVARIANT_TOL = 1e-13   # rounding only


# load-balance paths: default thresholds (no hubs / big rows on these small graphs) and
# lowered ones that send most pushes through the LDS hub table and the big-row kernel
# and the three iteration policies: never pull, always pull, pull only for large frontiers
TUNINGS = [dict(pull_min_frontier=-1), dict(hub_min_degree=3, big_row_edges=8, pull_min_frontier=-1),
           dict(hub_min_degree=1, big_row_edges=1, pull_min_frontier=-1), dict(pull_min_frontier=1),
           dict(hub_min_degree=3, big_row_edges=8, pull_min_frontier=40), dict(),
           dict(pull_min_frontier=40, chunk_iters=1), dict(hub_min_degree=3, pull_min_frontier=60, chunk_iters=3),
           dict(pull_min_frontier=1, pull_block=512, big_row_edges=8), dict(pull_min_frontier=30, pull_block=1024, big_row_edges=4),
           # resident sweeps (one launch per run of dense iterations) are on by default: also run
           # without them, with small workgroups (several groups), and with a roll-call that cannot
           # succeed (the first resident launch gives up untouched, per-iteration launches go on)
           dict(pull_min_frontier=1, persistent=0), dict(pull_min_frontier=1, pull_block=256),
           dict(pull_min_frontier=1, pull_block=256, persist_timeout_us=-1),
           # resident launches that may run only 3 sweeps at a time: every one stops mid-phase and is resumed
           dict(pull_min_frontier=1, chunk_iters=3),
           # per-iteration sweeps that test the activity bitmap before each gather (several groups / mixed with push / odd block)
           dict(pull_min_frontier=1, persistent=0, sweep_bitmap=1, pull_block=256, big_row_edges=8),
           dict(pull_min_frontier=40, persistent=0, sweep_bitmap=1), dict(pull_min_frontier=1, sweep_bitmap=1, pull_block=640),
           # binned sweeps (k_bin_scatter + k_bin_reduce instead of k_pull_iter; on by itself only on windows of millions of
           # vertices): one-tile blocks of ~64 edges (dozens of blocks, every tile a handful of edges), the default
           # block shape (one block each), and mixed with push iterations in chunks of 3
           dict(pull_min_frontier=1, persistent=0, binned=(2, 1, 1, 64, 0, 64, 64)), dict(pull_min_frontier=1, persistent=0, binned=2),
           dict(pull_min_frontier=40, persistent=0, binned=(2, 2, 3, 200, 0, 100, 500), chunk_iters=3),
           # the batch's records grouped by tail (and CopyOutDegree done) at slide time, outside the timed region (rounds 3-4; the
           # default since round 5 keeps both inside, where the reference times them)
           dict(group_at_slide=1), dict(pull_min_frontier=1, group_at_slide=1),
           # edge slots of the resident sweep in CSR order (rounds 1-2; the default is the table sorted by gather position), also
           # on several small groups
           dict(pull_min_frontier=1, resident_slots=0), dict(resident_slots=0, pull_block=256),
           # IncrementalBatchUpdate as a kernel of its own in front of a whole-batch resident launch (the default applies the
           # records inside the launch)
           dict(resident_update=0), dict(resident_update=0, pull_block=256)]
TUNING_IDS = ["push-only", "push-hubs+bigrows", "push-all-hub-all-big", "pull-only", "mixed-pull>=40", "default",
              "mixed-chunk1", "mixed-chunk3", "pull-wg512", "mixed-wg1024", "pull-no-persist", "pull-wg256",
              "pull-rollcall-fails", "pull-resident-3-sweeps", "pull-bitmap-wg256", "mixed-bitmap", "pull-bitmap-wg640",
              "binned-tiny-blocks", "binned-one-block", "mixed-binned-chunk3", "grouping-at-slide", "pull-grouping-at-slide",
              "resident-csr-slots", "resident-csr-slots-wg256", "resident-update-own-kernel", "resident-update-own-kernel-wg256"]


def make(directed, schedule=eng.SCHEDULE_EAGER, scale=9, edges=6000, seed=11, W=600, c=6, eps=1e-9, n_epochs=1,
         tuning=None):
    V, e1, e2 = datagen.rmat_stream(scale, edges, seed)
    src = int(datagen.top_sources(V, e1, e2, W, directed, 1)[0])
    return Scenario(V, e1, e2, directed, W, c, src, eps, schedule=schedule, n_epochs=n_epochs, **(tuning or {}))


def check_csr(sc):
    """Device CSR == host CSR (the -DVALIDATE check of gpu/PPRRevPushGPU.cuh:45-90)."""
    row, col, deg = sc.e.read_graph()
    orow, ocol = sc.g.flatten(1)
    assert np.array_equal(row, orow)
    assert np.array_equal(col, sorted_csr(orow, ocol))
    assert np.array_equal(deg, sc.g.deg())
    row, col = sc.e.read_out_graph()          # the out-CSR of the pull sweep
    orow, ocol = sc.g.flatten(0)
    assert np.array_equal(row, orow)
    assert np.array_equal(col, sorted_csr(orow, ocol))


@pytest.mark.parametrize("directed", [1, 0])
def test_device_csr_matches_host_every_slide(directed):
    sc = make(directed)
    check_csr(sc)
    for _ in range(12):           # slides wrap the ring (W=600, c=6 -> also W % c == 0 case below)
        assert sc.advance_graphs()
        check_csr(sc)


def test_device_csr_ring_wraparound_misaligned():
    sc = make(0, W=100, c=7, edges=2000)   # 100 % 7 != 0: a slide straddles the ring end
    for _ in range(40):
        assert sc.advance_graphs()
        check_csr(sc)


@pytest.mark.parametrize("phase", [0, 1])
def test_inspect_frontier_bit_exact(phase):
    sc = make(1)
    rng = np.random.default_rng(5)
    eps = sc.eps
    r = rng.normal(0, 2e-9, sc.V)
    r[::7] = eps            # exactly on the threshold: NOT legal (strict inequality)
    r[1::7] = -eps
    r[2::7] = np.nextafter(eps, 1)
    r[3::7] = np.nextafter(-eps, -1)
    sc.e.write(sc.slot, np.zeros(sc.V), r)
    sc.s.r[:] = r
    got = np.sort(sc.e.inspect(sc.slot, phase, eps))
    want = sc.s.inspect(phase)
    assert np.array_equal(got, want)
    # empty frontier
    sc.e.write(sc.slot, np.zeros(sc.V), np.zeros(sc.V))
    assert len(sc.e.inspect(sc.slot, phase, eps)) == 0


@pytest.mark.parametrize("at_slide", [1, 0])
@pytest.mark.parametrize("directed", [1, 0])
def test_incremental_batch_update_bit_exact(directed, at_slide):
    """r after IncrementalBatchUpdate == cpu/PPRCPUMTCilkRev.h:108-124 at -t 1, bit for bit (records grouped by tail when the
    batch is uploaded, or inside the call: dppr_set_batch_grouping)."""
    sc = make(directed, c=50, tuning=dict(group_at_slide=at_slide))
    sc.s.cilk_execute(sc.g)
    for k in range(4):
        sc.e.write(sc.slot, sc.s.p.copy(), sc.s.r.copy())
        assert sc.advance_graphs()
        sc.s.copy_revert_out_degree(sc.g)
        sc.s.stream_update(sc.g)
        sc.e.incremental_batch_update(sc.slot)
        p, r = sc.e.read(sc.slot)
        assert np.array_equal(r, sc.s.r), k
        assert np.array_equal(p, sc.s.p)
        # finish the batch on the oracle so the next round starts from a converged state
        sc.s.dyn_push_init(sc.g, 0); sc.s.cilk_main_loop(sc.g, 0)
        sc.s.dyn_push_init(sc.g, 1); sc.s.cilk_main_loop(sc.g, 1)


def test_incremental_batch_update_hub_tail_many_records():
    """A batch in which one tail owns most records (long sequential group)."""
    V, W, c = 64, 40, 20
    rng = np.random.default_rng(3)
    e1 = np.where(rng.random(400) < 0.7, 5, rng.integers(0, V, 400)).astype(np.int32)
    e2 = rng.integers(0, V, 400).astype(np.int32)
    e2 = np.where(e2 == e1, (e2 + 1) % V, e2).astype(np.int32)
    sc = Scenario(V, e1, e2, 1, W, c, 5, 1e-9)
    sc.s.cilk_execute(sc.g)
    sc.e.write(sc.slot, sc.s.p.copy(), sc.s.r.copy())
    assert sc.advance_graphs()
    sc.s.copy_revert_out_degree(sc.g)
    sc.s.stream_update(sc.g)
    sc.e.incremental_batch_update(sc.slot)
    _, r = sc.e.read(sc.slot)
    assert np.array_equal(r, sc.s.r)


@pytest.mark.parametrize("grouping", ["hand-written", "device-radix-sort"])
@pytest.mark.parametrize("shape", ["group-beyond-lds-window", "more-records-than-one-grid-pass", "hub-tail-in-a-large-batch"])
def test_incremental_batch_update_large_batches(shape, grouping, monkeypatch):
    """k_su_apply_fused stages 1024 sorted records per workgroup in LDS: a tail group longer than the window finishes
    from global memory. From 65 536 records on, the terms of all records are computed in parallel first and the group leaders
    walk contiguous arrays (k_su_terms + k_su_apply: a hub's tail owns thousands of records there), over several grid
    passes -- all still bit-identical to the CPU order. The records of these batches (12 000 / 540 000 / 120 000) are grouped inside the
    call by the hand-written bucket + rank kernels (round 6: k_su_grp_hist / _scatter / _rank; a hub tail of 36 000 records sits in ONE
    bucket) or -- the fallback for batches beyond 4 Mi records, DPPR_GROUPING_RADIX=1 -- by the device radix sort: same residuals."""
    if grouping == "device-radix-sort":
        monkeypatch.setenv("DPPR_GROUPING_RADIX", "1")
    rng = np.random.default_rng(7)
    if shape == "group-beyond-lds-window":
        V, W, c, n = 64, 4000, 3000, 12000          # 70 % of the records share tail 5: a ~4000-record group
        e1 = np.where(rng.random(n) < 0.7, 5, rng.integers(0, V, n)).astype(np.int32)
    elif shape == "hub-tail-in-a-large-batch":
        V, W, c, n = 4096, 200000, 60000, 400000    # L = 120 000; 30 % of the records share tail 5: a ~36 000-record group
        e1 = np.where(rng.random(n) < 0.3, 5, rng.integers(0, V, n)).astype(np.int32)
    else:
        V, W, c, n = 4096, 300000, 270000, 900000   # L = 2c = 540 000 > 524 288
        e1 = rng.integers(0, V, n).astype(np.int32)
    e2 = rng.integers(0, V, n).astype(np.int32)
    e2 = np.where(e2 == e1, (e2 + 1) % V, e2).astype(np.int32)
    sc = Scenario(V, e1, e2, 1, W, c, 5, 1e-9)
    sc.s.cilk_execute(sc.g)
    sc.e.write(sc.slot, sc.s.p.copy(), sc.s.r.copy())
    assert sc.advance_graphs()
    sc.s.copy_revert_out_degree(sc.g)
    sc.s.stream_update(sc.g)
    sc.e.incremental_batch_update(sc.slot)
    _, r = sc.e.read(sc.slot)
    assert np.array_equal(r, sc.s.r)


def _boundary_batch_update(L, V, hub_frac, at_slide, want_path):
    """One directed batch of exactly L records (c = ceil(L / 2) stream edges retired and inserted; an odd L drops the last insert
    record on both sides), from a random state written to the engine and the oracle alike: r after IncrementalBatchUpdate must equal
    the oracle's stream_update bit for bit. No environment switch: the grouping path is the one the batch selects by itself, read
    back first (dppr_debug_grouping) -- which must leave the batch's residuals untouched."""
    c = (L + 1) // 2
    W = c
    rng = np.random.default_rng(L + int(hub_frac * 100))
    n = W + c
    e1 = rng.integers(0, V, n)
    if hub_frac:
        e1 = np.where(rng.random(n) < hub_frac, 5, e1)
    e1 = e1.astype(np.int32)
    e2 = rng.integers(0, V, n).astype(np.int32)
    e2 = np.where(e2 == e1, (e2 + 1) % V, e2).astype(np.int32)
    sc = Scenario(V, e1, e2, 1, W, c, 5, 1e-9, group_at_slide=at_slide)
    p = rng.random(V) * 1e-3
    r = rng.normal(0.0, 1e-6, V)
    sc.e.write(sc.slot, p, r)
    sc.s.p[:] = p
    sc.s.r[:] = r
    assert not sc.g.stream_updates()
    sc.g.inc_construct(1)
    b1, b2, ins = sc.g.batch()
    assert len(b1) >= L
    sc.g._g.contents.blen = L                      # (the oracle replays its first L records; the window is the full slide's)
    sc.e.set_batch(b1[:L], b2[:L], ins[:L])
    sc.e.slide(*sc.g.new_stream())
    assert sc.e.debug_grouping(path=0)[3] == want_path
    sc.s.copy_revert_out_degree(sc.g)
    sc.s.stream_update(sc.g)
    sc.e.incremental_batch_update(sc.slot)
    _, r = sc.e.read(sc.slot)
    assert np.array_equal(r, sc.s.r)
    sc.e.close()


@pytest.mark.parametrize("L,path", [(4096, 1), (4097, 2), ((1 << 22) + 1, 3)], ids=["4096-rank", "4097-bucket", "4Mi+1-radix"])
def test_incremental_batch_update_at_grouping_boundaries(L, path):
    """The last length of the ranking launch, the first of the bucket path, and the first the radix sort takes by length alone."""
    _boundary_batch_update(L, 1 << 20 if L > 4097 else 4096, 0.0, 0, path)


@pytest.mark.parametrize("at_slide", [0, 1])
def test_incremental_batch_update_one_tail_million_records(at_slide):
    """1 Mi records, 90 % of them on one tail: grouped by the radix sort (the fullest bucket is far above SU_GRP_MAX_BUCKET), or at
    slide; k_su_apply walks a ~940 000-record group with the whole wave."""
    _boundary_batch_update(1 << 20, 1 << 16, 0.9, at_slide, 4 if at_slide else 3)


@pytest.mark.parametrize("tuning", TUNINGS, ids=TUNING_IDS)
@pytest.mark.parametrize("directed", [1, 0])
def test_sync_schedule_frontier_sets_bit_exact(directed, tuning):
    """Deterministic mode: every iteration's frontier SET equals the oracle's synchronous
    schedule; p/r agree to rounding of the atomic sums."""
    sc = make(directed, schedule=eng.SCHEDULE_SYNC, c=20, tuning=tuning)
    sc.s.trace(True)
    sc.e.trace_enable(sc.slot, True)
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)

    def compare():
        want = sc.s.traced_frontiers()
        got = sc.e.trace_get(sc.slot)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert np.array_equal(np.sort(a), np.sort(b))
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL
        assert np.max(np.abs(r - sc.s.r)) < SYNC_TOL

    compare()
    for _ in range(5):
        assert sc.advance_graphs()
        sc.s.trace(True)
        sc.e.trace_enable(sc.slot, True)
        sc.s.sync_inc_execute(sc.g)
        sc.e.update(sc.slot, sc.eps)
        compare()
    st = sc.e.stats(sc.slot)
    assert st["sum_E"] == sc.s.stats()["E"] and st["sum_F"] == sc.s.stats()["F"]
    if "binned" in tuning:   # every sweep took the binned form
        assert st["binned_sweeps"] == st["pull_iterations"] > 0
    else:
        assert st["binned_sweeps"] == 0


VARIANT_TUNINGS = [dict(), dict(hub_min_degree=3, big_row_edges=8, pull_min_frontier=-1), dict(hub_min_degree=1, big_row_edges=1, pull_min_frontier=-1),
                   dict(pull_min_frontier=40, persistent=0), dict(pull_min_frontier=40, chunk_iters=3)]
VARIANT_IDS = ["default", "hubs+bigrows", "all-hub-all-big", "mixed-with-sweeps", "mixed-resident-chunk3"]


@pytest.mark.parametrize("tuning", VARIANT_TUNINGS, ids=VARIANT_IDS)
@pytest.mark.parametrize("variant", [1, 3])
@pytest.mark.parametrize("directed", [1, 0])
def test_sync_schedule_is_the_reference_fast_frontier_variant(directed, variant, tuning):
    """`./pagerank -o 1|3` = dppr_set_variant(1 FAST_FRONTIER | 3 VANILLA): residuals pre-extracted and zeroed at the snapshot
    (InspectExtra), duplicates filtered by the threshold crossing (1) or the status array (3), no repair -- the reference's
    mechanisms (gpu/PPRRevPushGPUVariants.cuh:58-150) in the push kernels, on the synchronous schedule. Per-iteration frontier
    sets, iteration count and traversed edges equal the oracle's restatement of PPRCPUMTCilkRevFF / ...Vanilla
    (cpu/PPRCPUMTCilkRevVariants.h) at -t 1, batch after batch, also through hub tables, big rows and between sweeps."""
    sc = make(directed, c=20, tuning=dict(tuning, variant=variant))
    sc.s.trace(True)
    sc.e.trace_enable(sc.slot, True)
    sc.s.variant_execute(sc.g, variant)
    sc.e.init_solve(sc.slot, sc.eps)
    for k in range(5):
        if k:
            assert sc.advance_graphs()
            sc.s.trace(True)
            sc.e.trace_enable(sc.slot, True)
            sc.s.variant_inc_execute(sc.g, variant)
            sc.e.update(sc.slot, sc.eps)
        want, got = sc.s.traced_frontiers(), sc.e.trace_get(sc.slot)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert np.array_equal(np.sort(a), np.sort(b))
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL
    st, want = sc.e.stats(sc.slot), sc.s.stats()
    assert (st["iterations"], st["sum_F"], st["sum_E"]) == (want["iters"], want["F"], want["E"])


@pytest.mark.parametrize("tuning", TUNINGS, ids=TUNING_IDS)
@pytest.mark.parametrize("directed", [1, 0])
def test_sync_schedule_chunked_launches_same_work(directed, tuning):
    """Without the frontier trace the loop enqueues iterations in chunks (one host read-back per
    chunk). The synchronous schedule must still do exactly the oracle's work: same number of
    iterations, same sum of frontier sizes, same traversed edges, p/r to rounding."""
    sc = make(directed, schedule=eng.SCHEDULE_SYNC, c=20, tuning=tuning)
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)
    for k in range(5):
        if k:
            assert sc.advance_graphs()
            sc.s.sync_inc_execute(sc.g)
            sc.e.update(sc.slot, sc.eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL
        st, want = sc.e.stats(sc.slot), sc.s.stats()
        assert (st["iterations"], st["sum_F"], st["sum_E"]) == (want["iters"], want["F"], want["E"])


@pytest.mark.parametrize("tuning", TUNINGS, ids=TUNING_IDS)
@pytest.mark.parametrize("eps", [1e-9, 1e-6])
@pytest.mark.parametrize("directed", [1, 0])
def test_eager_schedule_parity_with_cilk_oracle(directed, eps, tuning):
    """Production mode against the cpu/PPRCPUMTCilkRev restatement: north-star tolerance,
    plus the reference's Validate() criteria and the loop invariant."""
    sc = make(directed, c=30, eps=eps, tuning=tuning)
    sc.s.cilk_execute(sc.g)
    sc.e.init_solve(sc.slot, eps)
    for k in range(6):
        if k:
            assert sc.advance_graphs()
            sc.s.cilk_inc_execute(sc.g)
            sc.e.update(sc.slot, eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(r)) < eps                                  # gpu/PPRRevPushGPU.cuh:141-143
        pw, _ = orc.pow_rev(sc.g, sc.source)
        assert np.max(np.abs(p - pw)) < 100 * eps                        # gpu/PPRRevPushGPU.cuh:145-156
        tol = NORTH_STAR_TOL * (eps / 1e-9)
        assert np.max(np.abs(p - sc.s.p)) < tol
        assert np.max(np.abs(r - sc.s.r)) < 2 * eps                      # both lie in (-eps, eps)
        src, dst = window_directed_edges(sc.g)
        assert invariant_max_err_np(p, r, src, dst, sc.V, sc.source) < INVARIANT_TOL


@pytest.mark.parametrize("schedule", ["sync", "eager"])
@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("directed", [1, 0])
def test_single_edge_batches(directed, c, schedule):
    """The reference's smallest experiment point, scripts/gpu.sh:13 (batch size c = 1: one deleted and one inserted
    edge per batch, L = 2 records directed / 4 undirected): 25 batches in a row, device CSR every slide, synchronous
    schedule with the oracle's frontier sets / statistics, production schedule within the north-star tolerance."""
    sync = schedule == "sync"
    sc = make(directed, schedule=eng.SCHEDULE_SYNC if sync else eng.SCHEDULE_EAGER, c=c, W=600)
    if sync:
        sc.s.sync_execute(sc.g)
    else:
        sc.s.cilk_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)
    for k in range(25):
        assert sc.advance_graphs()
        if sync:
            sc.s.sync_inc_execute(sc.g)
        else:
            sc.s.cilk_inc_execute(sc.g)
        sc.e.update(sc.slot, sc.eps)
        if k % 6 == 0:
            check_csr(sc)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(r)) < sc.eps
        if sync:
            assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL, k
        else:
            assert np.max(np.abs(p - sc.s.p)) < NORTH_STAR_TOL, k
    if sync:
        st, want = sc.e.stats(sc.slot), sc.s.stats()
        assert (st["iterations"], st["sum_F"], st["sum_E"]) == (want["iters"], want["F"], want["E"])


@pytest.mark.parametrize("eps", [1e-5, 1e-10])
@pytest.mark.parametrize("directed", [1, 0])
def test_epsilon_sweep_corners(directed, eps):
    """The ends of the reference's epsilon sweep, scripts/gpu.sh:83 (1e-5 .. 1e-10): the synchronous schedule does the
    oracle's work exactly (iterations, sum F, sum E), the production schedule stays within the tolerance scaled as
    test_eager_schedule_parity_with_cilk_oracle scales it, |r| < eps and the reference's Validate() bound hold."""
    for sync in (True, False):
        sc = make(directed, schedule=eng.SCHEDULE_SYNC if sync else eng.SCHEDULE_EAGER, c=30, eps=eps)
        if sync:
            sc.s.sync_execute(sc.g)
        else:
            sc.s.cilk_execute(sc.g)
        sc.e.init_solve(sc.slot, eps)
        for k in range(5):
            if k:
                assert sc.advance_graphs()
                if sync:
                    sc.s.sync_inc_execute(sc.g)
                else:
                    sc.s.cilk_inc_execute(sc.g)
                sc.e.update(sc.slot, eps)
            p, r = sc.e.read(sc.slot)
            assert np.max(np.abs(r)) < eps
            pw, _ = orc.pow_rev(sc.g, sc.source)
            assert np.max(np.abs(p - pw)) < 100 * eps
            if sync:
                assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL
            else:
                assert np.max(np.abs(p - sc.s.p)) < max(NORTH_STAR_TOL * (eps / 1e-9), 1e-12)
        if sync:
            st, want = sc.e.stats(sc.slot), sc.s.stats()
            assert (st["iterations"], st["sum_F"], st["sum_E"]) == (want["iters"], want["F"], want["E"])
        sc.e.close()


@pytest.mark.parametrize("eps", [1e-5, 1e-10])
@pytest.mark.parametrize("c", [1, 40])
def test_source_group_batch_size_and_epsilon_corners(c, eps):
    """The same corners for a source group (10 sources, 80-byte rows): single-edge batches and both ends of the epsilon
    sweep, per-source p / r of the oracle's synchronous schedule and its summed statistics."""
    V, e1, e2 = datagen.rmat_stream(10, 9000, 5)
    W, directed = 1500, 1
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 10)]
    run_source_group(V, e1, e2, W, c, eps, directed, sources, 8 if c == 1 else 4, "tails")


def test_split_interface_matches_reference_driver_flow():
    """IncrementalBatchUpdate + ExecuteMainLoop(0) + ExecuteMainLoop(1) called separately
    (full Inspect seeding, gpu/PPRRevPushGPU.cuh:97-131) gives the same frontier sets as the
    fused dppr_update in the synchronous schedule."""
    a = make(1, schedule=eng.SCHEDULE_SYNC, c=20)
    b = make(1, schedule=eng.SCHEDULE_SYNC, c=20)
    a.e.init_solve(a.slot, a.eps)
    b.e.init_solve(b.slot, b.eps)
    for _ in range(3):
        assert a.advance_graphs() and b.advance_graphs()
        a.e.trace_enable(a.slot, True)
        b.e.trace_enable(b.slot, True)
        a.e.update(a.slot, a.eps)
        b.e.incremental_batch_update(b.slot)
        b.e.execute_main_loop(b.slot, 0, b.eps)
        b.e.execute_main_loop(b.slot, 1, b.eps)
        fa, fb = a.e.trace_get(a.slot), b.e.trace_get(b.slot)
        assert len(fa) == len(fb)
        for x, y in zip(fa, fb):
            assert np.array_equal(np.sort(x), np.sort(y))


# The reference's own incremental window graph is wrong on this one fixture (quirk Q1, tests/test_oracle_golden.py::
# test_quirk_q1_inc_construct_undirected_misaligned: undirected stream, W % c != 0 -- IncConstructWindowGraph expires mirrored records by
# count from the list front and transiently holds another multiset of edges than the window), so the p its FIFO run left in the
# fixture belongs to a different graph than the stream's; the engine is held to the from-scratch power iteration there.
REFERENCE_GRAPH_QUIRK = {"und_long_misaligned_e9"}


@pytest.mark.parametrize("name", golden_names())
def test_golden_fixtures_reference_ground_truth(name):
    """Engine vs vectors computed by the REAL reference (power iteration + FIFO push), at the bound the mathematics gives.
    Any state with the loop invariant p + a r = a e_s + M p (M = (1-a) D^-1 A over outdeg + 1, row sums < 1 - a) satisfies
    p - p* = -a (I - M)^-1 r, and |(I - M)^-1|_inf <= 1 / a: every state with |r| < eps lies within eps of the fixed point,
    the engine's and the reference's FIFO state within 2 eps of each other (round 4 asserted 200 eps). Measured on these
    fixtures: 0.18 - 0.28 eps (printed with -s)."""
    d, m = load_golden(name)
    eps = m["eps"]
    sc = Scenario(m["V"], d["stream.e1"], d["stream.e2"], m["directed"], m["W"], m["c"], m["source"], eps)
    sc.e.init_solve(sc.slot, eps)
    worst = 0.0
    for k in range(0, min(m["done"], 12) + 1):
        if k:
            assert sc.advance_graphs()
            sc.e.update(sc.slot, eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(r)) < eps
        assert np.max(np.abs(p - d[f"b{k}.pow.p"])) < 100 * eps      # (the reference's own Validate() bound against its power iteration)
        if name in REFERENCE_GRAPH_QUIRK and k > 0:
            continue
        dev = float(np.max(np.abs(p - d[f"b{k}.fifo.p"])))
        worst = max(worst, dev)
        assert dev < 2 * eps, (f"batch {k}: |p_engine - p_reference_fifo| = {dev / eps:.2f} eps; both states have |r| < eps and must lie within "
                               f"eps of the fixed point each")
    print(f"{name}: max |p_engine - p_reference_fifo| = {worst / eps:.3f} eps")
    assert (name in REFERENCE_GRAPH_QUIRK) == (not m["directed"] and m["W"] % m["c"] != 0 and m["done"] > 12)   # the quirk's condition, stated once


def test_edge_cases():
    eps = 1e-9
    # source without in-edges: the frontier dies after one iteration; p[s] = alpha
    V = 16
    e1 = np.array([0, 0, 1, 2, 3, 4, 5, 6], dtype=np.int32)
    e2 = np.array([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.int32)
    sc = Scenario(V, e1, e2, 1, 4, 2, 0, eps)
    sc.e.init_solve(sc.slot, eps)
    p, r = sc.e.read(sc.slot)
    assert p[0] == 0.15 and np.count_nonzero(p) == 1 and np.all(r == 0)
    # slide twice then hit the end of the stream (partial batch is dropped by the host side)
    for _ in range(2):
        assert sc.advance_graphs()
        sc.e.update(sc.slot, eps)                 # (epochs are applied in sequence: no skipping)
    assert not sc.advance_graphs()
    # empty batch: update is a no-op
    sc.e.set_batch(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8))
    sc.e.slide(np.zeros(0, np.int32), np.zeros(0, np.int32))
    before = sc.e.read(sc.slot)
    sc.e.update(sc.slot, eps)
    after = sc.e.read(sc.slot)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # self loops and duplicate edges
    e1 = np.array([1, 1, 1, 2, 2, 3, 3, 3, 1, 2, 3, 1], dtype=np.int32)
    e2 = np.array([1, 2, 2, 1, 2, 1, 3, 1, 3, 3, 2, 1], dtype=np.int32)
    sc = Scenario(4, e1, e2, 1, 6, 2, 1, eps)
    sc.s.cilk_execute(sc.g)
    sc.e.init_solve(sc.slot, eps)
    for k in range(3):
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < NORTH_STAR_TOL and np.max(np.abs(r)) < eps
        if not sc.advance_graphs():
            break
        sc.s.cilk_inc_execute(sc.g)
        sc.e.update(sc.slot, eps)


@pytest.mark.parametrize("directed", [1, 0])
def test_seed_lists_equal_dyn_push_init(directed):
    """The one iteration where the reference's CPU schedule and this engine coincide exactly: the
    frontier after the stream update. The lists IncrementalBatchUpdate emits (phase 0: tails with
    r > eps; phase 1 candidates: tails with r < -eps) must be the sets DynPushInit builds from the
    batch endpoints (cpu/PPRCPUMTCilkRev.h:126-156), for every batch."""
    sc = make(directed, c=40)
    sc.s.cilk_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)
    for k in range(6):
        assert sc.advance_graphs()
        # oracle: update, then both seed sets read off the updated residuals
        sc.s.copy_revert_out_degree(sc.g)
        sc.s.stream_update(sc.g)
        want = []
        for phase in (0, 1):
            sc.s.dyn_push_init(sc.g, phase)
            want.append(np.sort(sc.s.frontier()))
        sc.e.incremental_batch_update(sc.slot)
        for phase in (0, 1):
            got = np.sort(sc.e.seed_lists(sc.slot, phase))
            assert np.array_equal(got, want[phase]), (k, phase)
            assert np.array_equal(got, sc.s.inspect(phase))            # == a full Inspect pass (gpu/Inspect.cuh:8-48)
        # finish the batch on both sides (the engine through the reference's split driver flow)
        sc.s.dyn_push_init(sc.g, 0); sc.s.cilk_main_loop(sc.g, 0)
        sc.s.dyn_push_init(sc.g, 1); sc.s.cilk_main_loop(sc.g, 1)
        sc.e.execute_main_loop(sc.slot, 0, sc.eps)
        sc.e.execute_main_loop(sc.slot, 1, sc.eps)
        with pytest.raises(eng.DpprError):
            sc.e.seed_lists(sc.slot, 0)                                  # only valid right after the update
        p, _ = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < NORTH_STAR_TOL


def test_epochs_must_be_applied_in_sequence_and_slide_is_bounded():
    K = 4
    sc = make(1, c=20, n_epochs=K + 1)
    gid = sc.e.add_source_group([sc.source, int((sc.source + 1) % sc.V)])
    sc.e.init_solve(sc.slot, sc.eps)
    sc.e.group_init_solve(gid, sc.eps)
    for _ in range(K):
        assert sc.advance_graphs()
    with pytest.raises(eng.DpprError):
        sc.e.update(sc.slot, sc.eps, epoch=2)        # epoch 1 skipped
    sc.e.update(sc.slot, sc.eps, epoch=1)
    with pytest.raises(eng.DpprError):
        sc.e.update(sc.slot, sc.eps, epoch=1)        # replayed
    with pytest.raises(eng.DpprError):
        sc.e.update(sc.slot, sc.eps, epoch=3)        # epoch 2 skipped
    with pytest.raises(eng.DpprError):
        sc.e.group_update(gid, sc.eps, epoch=2)
    for k in range(1, K + 1):
        sc.e.group_update(gid, sc.eps, epoch=k)
        if k > 1:
            sc.e.update(sc.slot, sc.eps, epoch=k)
    p, r = sc.e.read(sc.slot)
    pg, rg = sc.e.group_read(gid, 0)
    assert np.max(np.abs(p - pg)) < NORTH_STAR_TOL and np.max(np.abs(r)) < sc.eps
    # a slide longer than max_batch of dppr_create is refused (its key buffers are sized for max_batch)
    n = sc.c + 1
    sc.e.set_batch(np.zeros(2 * n, np.int32), np.ones(2 * n, np.int32), np.zeros(2 * n, np.uint8))
    with pytest.raises(eng.DpprError):
        sc.e.slide(np.zeros(n, np.int32), np.ones(n, np.int32))


def test_error_paths():
    sc = make(1)
    with pytest.raises(eng.DpprError):
        sc.e.update(99, 1e-9)                     # bad slot
    with pytest.raises(eng.DpprError):
        sc.e.update(sc.slot, 1e-9, epoch=7)       # epoch never built
    with pytest.raises(eng.DpprError):
        sc.e.add_source(sc.V)                     # vertex out of range
    with pytest.raises(eng.DpprError):
        sc.e.load_window(np.zeros(3, np.int32), np.zeros(3, np.int32))  # n != W


def test_rejected_calls_change_nothing():
    """A call that returns DPPR_ERR_INVALID is a no-op: ids out of range are detected BEFORE any id is assigned, any parked
    vertex revived or any epoch dropped -- the stream goes on afterwards as if the call had not been made."""
    sc = make(1, c=10)
    sc.s.cilk_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)
    g = sc.g._g.contents
    seen = np.zeros(sc.V, bool)
    seen[np.ctypeslib.as_array(g.s1, (g.stream_len,))[:g.pos]] = True
    seen[np.ctypeslib.as_array(g.s2, (g.stream_len,))[:g.pos]] = True
    fresh = np.nonzero(~seen)[0][:4].astype(np.int32)   # vertices without an id: a valid prefix of the rejected arrays
    before = sc.e.id_space()
    bad = np.concatenate([fresh, np.array([sc.V], np.int32)])
    with pytest.raises(eng.DpprError):
        sc.e.set_batch(bad, np.zeros(5, np.int32), np.ones(5, np.uint8))
    with pytest.raises(eng.DpprError):
        sc.e.slide(bad, np.zeros(5, np.int32))
    with pytest.raises(eng.DpprError):
        sc.e.slide(np.zeros(5, np.int32), np.concatenate([fresh, np.array([-1], np.int32)]))
    with pytest.raises(eng.DpprError):
        sc.e.add_source_group(bad)
    assert sc.e.id_space() == before
    for _ in range(3):                                   # the newest epoch is still there, the stream goes on
        assert sc.advance_graphs()
        sc.s.cilk_inc_execute(sc.g)
        sc.e.update(sc.slot, sc.eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < NORTH_STAR_TOL and np.max(np.abs(r)) < sc.eps
    check_csr(sc)


def test_multi_epoch_prestaging_and_two_sources():
    """K epochs staged in HBM first, then the timed path run back to back; two sources share the graph."""
    K = 5
    sc = make(0, c=25, n_epochs=K + 1)
    slot2 = sc.e.add_source(int((sc.source + 1) % sc.V))
    s2 = orc.State(sc.V, int((sc.source + 1) % sc.V), sc.eps)
    sc.e.init_solve(sc.slot, sc.eps)
    sc.e.init_solve(slot2, sc.eps)
    sc.s.cilk_execute(sc.g)
    s2.cilk_execute(sc.g)
    want = []
    for k in range(1, K + 1):
        assert sc.advance_graphs()
        sc.s.cilk_inc_execute(sc.g)
        s2.cilk_inc_execute(sc.g)
        want.append((sc.s.p.copy(), s2.p.copy()))
    for k in range(1, K + 1):
        sc.e.update(sc.slot, sc.eps, epoch=k)
        sc.e.update(slot2, sc.eps, epoch=k)
        p1, _ = sc.e.read(sc.slot)
        p2, _ = sc.e.read(slot2)
        assert np.max(np.abs(p1 - want[k - 1][0])) < NORTH_STAR_TOL
        assert np.max(np.abs(p2 - want[k - 1][1])) < NORTH_STAR_TOL
    with pytest.raises(eng.DpprError):
        sc.e.update(sc.slot, sc.eps, epoch=K + 7)


def test_binned_sweep_covers_ids_assigned_after_its_tables_were_built():
    """Epochs staged BEFORE a source outside the window receives its id: their binned tables cover fewer ids than their
    sweeps must (k_bin_reduce's extra workgroups take the new ids, which have no edge in those epochs). Both sources
    against the oracle through the staged epochs, synchronous schedule (frontier work equal, p / r to rounding)."""
    K = 3
    tuning = dict(pull_min_frontier=1, persistent=0, binned=(2, 1, 1, 64, 0, 64, 64))
    sc = make(1, schedule=eng.SCHEDULE_SYNC, c=20, n_epochs=K + 1, tuning=tuning)
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)
    want = []
    for k in range(1, K + 1):
        assert sc.advance_graphs()
        sc.s.sync_inc_execute(sc.g)
        want.append((sc.s.p.copy(), sc.s.r.copy()))
    used = np.zeros(sc.V, bool)
    g = sc.g._g.contents
    used[np.ctypeslib.as_array(g.s1, (g.stream_len,))[:g.pos]] = True
    used[np.ctypeslib.as_array(g.s2, (g.stream_len,))[:g.pos]] = True
    lonely = int(np.nonzero(~used)[0][0])            # never seen by the engine: gets a fresh id now
    ids0 = sc.e.id_space()["ids"]
    slot2 = sc.e.add_source(lonely)
    assert sc.e.id_space()["ids"] == ids0 + 1
    for k in range(1, K + 1):
        sc.e.update(sc.slot, sc.eps, epoch=k)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - want[k - 1][0])) < SYNC_TOL and np.max(np.abs(r - want[k - 1][1])) < SYNC_TOL
    st, w = sc.e.stats(sc.slot), sc.s.stats()
    assert (st["iterations"], st["sum_F"], st["sum_E"]) == (w["iters"], w["F"], w["E"]) and st["binned_sweeps"] == st["pull_iterations"] > 0
    sc.e.init_solve(slot2, sc.eps)                   # a source without an edge: one push, p = alpha at the source
    p2, r2 = sc.e.read(slot2)
    assert p2[lonely] == 0.15 and np.count_nonzero(p2) == 1 and not r2.any()
    assert sc.e.stats(slot2)["binned_sweeps"] == 1


def test_full_size_youtube_standin_properties():
    """BASELINE.json configs[1] size (com-youtube stand-in): size-independent properties --
    residual bound, loop invariant, stats consistency -- after init and 3 batches."""
    V, e1, e2, cfg = datagen.stand_in_stream("youtube", "/tmp/dppr_data")
    W, c, _, _ = orc.workload_config(len(e1), 0.1, 0, 0.01, 100, 0, 0)
    src = int(datagen.top_sources(V, e1, e2, W, cfg.directed, 1)[0])
    eps = 1e-9
    e = eng.Engine(V, W, cfg.directed, c)
    e.load_window(e1[:W], e2[:W])
    slot = e.add_source(src)
    e.init_solve(slot, eps)
    pos = W
    for k in range(4):
        if k:
            b1 = np.concatenate([e1[pos - W:pos - W + c], e1[pos:pos + c]])
            b2 = np.concatenate([e2[pos - W:pos - W + c], e2[pos:pos + c]])
            ins = np.concatenate([np.zeros(c, np.uint8), np.ones(c, np.uint8)])
            e.set_batch(np.concatenate([b1, b2]), np.concatenate([b2, b1]), np.concatenate([ins, ins]))
            e.slide(e1[pos:pos + c], e2[pos:pos + c])
            pos += c
            e.update(slot, eps)
        p, r = e.read(slot)
        assert np.max(np.abs(r)) < eps
        w1, w2 = e1[pos - W:pos], e2[pos - W:pos]
        s_, d_ = np.concatenate([w1, w2]), np.concatenate([w2, w1])
        assert invariant_max_err_np(p, r, s_, d_, V, src) < INVARIANT_TOL
        assert p[src] >= 0.15
    st = e.stats(slot)
    assert st["batches"] == 3 and st["sum_E"] > 0 and st["algorithmic_bytes"] > 16 * V * 3


def test_full_size_resident_sweeps_match_per_iteration_launches():
    """configs[1] size, 242 workgroups on all XCDs: resident launches (data-flow synchronised sweeps,
    both phases of a batch enqueued ahead) against per-iteration launches of the same engine code,
    batch by batch. The two evaluate the same sums in different orders, so p / r agree to rounding;
    a value read one iteration too early or too late would show up at ~1e-7."""
    V, e1, e2, cfg = datagen.stand_in_stream("youtube", "/tmp/dppr_data")
    W, c, _, _ = orc.workload_config(len(e1), 0.1, 0, 0.01, 100, 0, 0)
    src = int(datagen.top_sources(V, e1, e2, W, cfg.directed, 1)[0])
    eps = 1e-9
    engines = [eng.Engine(V, W, cfg.directed, c, persistent=m) for m in (0, 1)]
    slots = []
    for e in engines:
        e.load_window(e1[:W], e2[:W])
        slots.append(e.add_source(src))
        e.init_solve(slots[-1], eps)
    pos = W
    for k in range(16):
        if k:
            b1 = np.concatenate([e1[pos - W:pos - W + c], e1[pos:pos + c]])
            b2 = np.concatenate([e2[pos - W:pos - W + c], e2[pos:pos + c]])
            ins = np.concatenate([np.zeros(c, np.uint8), np.ones(c, np.uint8)])
            for e, sl in zip(engines, slots):
                e.set_batch(np.concatenate([b1, b2]), np.concatenate([b2, b1]), np.concatenate([ins, ins]))
                e.slide(e1[pos:pos + c], e2[pos:pos + c])
                e.update(sl, eps)
            pos += c
        (p0, r0), (p1, r1) = (e.read(sl) for e, sl in zip(engines, slots))
        assert np.max(np.abs(p0 - p1)) < 1e-13 and np.max(np.abs(r0 - r1)) < 1e-13, k
    st0, st1 = (e.stats(sl) for e, sl in zip(engines, slots))
    assert (st0["iterations"], st0["sum_F"], st0["sum_E"]) == (st1["iterations"], st1["sum_F"], st1["sum_E"])
    assert st0["persist_launches"] == 0 and st1["persist_launches"] >= 15 and st1["persist_aborts"] == 0


def test_update_inside_the_resident_launch_equals_the_update_kernel():
    """configs[1] size: IncrementalBatchUpdate applied by the resident launch itself (PLAN_UPDATE, the default) against the
    same engine with the update as its own kernel (k_su_apply_fused), batch by batch: the records are applied per tail in
    the same order with the same expressions, so the states agree to the rounding of the sweeps' LDS sums; iterations,
    frontier sizes and traversed edges are equal; the records are counted once; and a launch whose roll-call fails
    (nothing changed) is followed by the update kernel."""
    V, e1, e2, cfg = datagen.stand_in_stream("youtube", "/tmp/dppr_data")
    W, c, _, _ = orc.workload_config(len(e1), 0.1, 0, 0.01, 100, 0, 0)
    src = int(datagen.top_sources(V, e1, e2, W, cfg.directed, 1)[0])
    eps = 1e-9
    engines = [eng.Engine(V, W, cfg.directed, c, resident_update=m) for m in (0, 1)]   # (1: the default -- the launch takes the records RAW)
    engines.append(eng.Engine(V, W, cfg.directed, c, persist_timeout_us=-1))   # every roll-call fails
    engines.append(eng.Engine(V, W, cfg.directed, c, group_at_slide=1))        # records grouped at slide time, ranges per sweep group
    slots = []
    for e in engines:
        e.load_window(e1[:W], e2[:W])
        slots.append(e.add_source(src))
        e.init_solve(slots[-1], eps)
    pos = W
    for k in range(1, 9):
        b1 = np.concatenate([e1[pos - W:pos - W + c], e1[pos:pos + c]])
        b2 = np.concatenate([e2[pos - W:pos - W + c], e2[pos:pos + c]])
        ins = np.concatenate([np.zeros(c, np.uint8), np.ones(c, np.uint8)])
        for e, sl in zip(engines, slots):
            e.set_batch(np.concatenate([b1, b2]), np.concatenate([b2, b1]), np.concatenate([ins, ins]))
            e.slide(e1[pos:pos + c], e2[pos:pos + c])
            e.update(sl, eps)
        pos += c
        (p0, r0), (p1, r1), (p2, r2), (p3, r3) = (e.read(sl) for e, sl in zip(engines, slots))
        assert np.max(np.abs(p0 - p1)) < 1e-13 and np.max(np.abs(r0 - r1)) < 1e-13, k
        assert np.max(np.abs(p0 - p2)) < 1e-13 and np.max(np.abs(r0 - r2)) < 1e-13, k
        assert np.max(np.abs(p0 - p3)) < 1e-13 and np.max(np.abs(r0 - r3)) < 1e-13, k   # (raw and pre-grouped records: same terms, same order per tail)
    st0, st1, st2, st3 = (e.stats(sl) for e, sl in zip(engines, slots))
    for st in (st1, st2, st3):
        assert (st0["iterations"], st0["sum_F"], st0["sum_E"], st0["records"]) == (st["iterations"], st["sum_F"], st["sum_E"], st["records"])
    assert st1["persist_launches"] >= 8 and st1["persist_aborts"] == 0   # (the from-scratch solve's launches count too)
    assert st3["persist_launches"] == st1["persist_launches"] and st3["persist_aborts"] == 0
    assert st2["persist_aborts"] == 1
    for e in engines:
        e.close()


@pytest.mark.parametrize("directed", [1, 0])
def test_resident_launch_calls_itself_off_when_a_group_owns_too_many_records(directed):
    """Default accounting: the whole-batch resident launch takes the batch's records raw and every sweep group applies its own.
    Here every inserted edge has the same tail, so one 256-thread sweep group owns 300 records of a batch: the launch calls
    itself off before anything is changed (NOT a residency failure: no abort is counted, resident launches stay on), the update
    runs as its own kernels, the next batches do so at once -- and every state equals that of an engine whose update is always a
    kernel of its own, and the -t 1 oracle's within the north-star tolerance."""
    V, W, c, eps = 512, 600, 300, 1e-9
    rng = np.random.default_rng(3)
    e1, e2 = rng.integers(0, V, 6000).astype(np.int32), rng.integers(0, V, 6000).astype(np.int32)
    e1[W:] = 5
    e2[e2 == e1] = (e1[e2 == e1] + 1) % V
    scs = [Scenario(V, e1, e2, directed, W, c, 5, eps, pull_min_frontier=1, pull_block=256, **kw) for kw in (dict(), dict(resident_update=0))]
    sc, ref = scs
    for x in scs:
        x.e.init_solve(x.slot, eps)
    sc.s.cilk_execute(sc.g)
    for k in range(6):
        for x in scs:
            assert x.advance_graphs()
            x.e.update(x.slot, eps)
        (p0, r0), (p1, r1) = sc.e.read(sc.slot), ref.e.read(ref.slot)
        assert np.max(np.abs(p0 - p1)) < 1e-13 and np.max(np.abs(r0 - r1)) < 1e-13, k
        sc.s.cilk_inc_execute(sc.g)
        assert np.max(np.abs(p0 - sc.s.p)) < NORTH_STAR_TOL and np.max(np.abs(r0)) < eps, k
    st, st_ref = sc.e.stats(sc.slot), ref.e.stats(ref.slot)
    assert st["persist_aborts"] == 0 and st["records"] == st_ref["records"]
    assert st["persist_launches"] > st_ref["persist_launches"]   # (the launch that called itself off is counted as a launch)
    for x in scs:
        x.e.close()


def test_full_size_livejournal_standin_two_sources():
    """BASELINE.json configs[2] size (soc-LiveJournal1 stand-in, directed, 69 M stream edges):
    two sources drawn from degree ranks [10, 1000) share one device graph; size-independent
    properties after the from-scratch solve and two batches each."""
    from dynamicppr_amd import stream as st
    V, e1, e2, cfg = datagen.stand_in_stream("livejournal", "/tmp/dppr_data")
    wl = st.workload_config(len(e1), 0.1, 0, 0.01, 100)
    W, c = wl.window, wl.per_batch
    ranked = datagen.top_sources(V, e1, e2, W, cfg.directed, 1000)
    sources = [int(ranked[10]), int(ranked[500])]
    eps = 1e-9
    e = eng.Engine(V, W, cfg.directed, c)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    slots = [e.add_source(s) for s in sources]
    for sl in slots:
        e.init_solve(sl, eps)
    for k in range(3):
        if k:
            assert not ss.stream_updates()
            e.set_batch(*ss.batch_arrays())
            e.slide(*ss.new_arrays())
            for sl in slots:
                e.update(sl, eps)
        w1, w2 = ss.serialize_edge_stream()
        for sl, src in zip(slots, sources):
            p, r = e.read(sl)
            assert np.max(np.abs(r)) < eps
            assert invariant_max_err_np(p, r, w1, w2, V, src) < INVARIANT_TOL
            assert p[src] >= 0.15
    st0 = e.stats(slots[0])
    assert st0["batches"] == 2 and st0["pull_iterations"] > 0 and st0["sum_E"] > 10 * len(w1)


@pytest.mark.parametrize("mode", ["resident", "per-iteration", "rollcall-fails", "rollcall-fails-whole-batch", "heavy-groups",
                                  "csr-slots", "heavy-groups-csr-slots"])
@pytest.mark.parametrize("directed", [1, 0])
def test_resident_sweeps_same_work_as_per_iteration_launches(directed, mode):
    """Runs of dense iterations as ONE resident launch (k_pull_resident) do exactly the oracle's
    synchronous work -- iterations, sum of frontier sizes, traversed edges, p/r to rounding -- as do
    per-iteration launches, a resident launch whose roll-call fails (not co-resident: it gives up
    before touching anything), and groups with more edges than the kernel keeps in registers (edge
    slots beyond PERSIST_SLOTS)."""
    tuning = dict(pull_min_frontier=1)
    scale, edges, W, c = 10, 30000, 3000, 60
    if mode == "per-iteration":
        tuning["persistent"] = 0
    elif mode == "rollcall-fails":
        tuning["persist_timeout_us"] = -1
    elif mode == "rollcall-fails-whole-batch":
        # automatic push/pull threshold: the from-scratch solve stays sparse on this small graph, so the
        # first resident launch is a whole batch (seeding inside the kernel) -- and it has to put back
        # what it seeded when its roll-call fails
        tuning = dict(persist_timeout_us=-1)
    elif mode.startswith("heavy-groups"):
        tuning["pull_block"] = 256
        edges, W, c = 200000, 40000, 400 # ~80 edges per vertex: a 256-vertex group carries > 4 * 256 edges
    if mode.endswith("csr-slots"):
        tuning["resident_slots"] = 0     # slots in CSR order (the default is the sorted slot table)
    V, e1, e2 = datagen.rmat_stream(scale, edges, 21)
    src = int(datagen.top_sources(V, e1, e2, W, directed, 1)[0])
    sc = Scenario(V, e1, e2, directed, W, c, src, 1e-9, schedule=eng.SCHEDULE_SYNC, **tuning)
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)
    for k in range(4):
        if k:
            assert sc.advance_graphs()
            sc.s.sync_inc_execute(sc.g)
            sc.e.update(sc.slot, sc.eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL
    stats = sc.e.stats(sc.slot)
    want = sc.s.stats()
    assert stats["iterations"] == want["iters"]
    assert stats["sum_F"] == want["F"] and stats["sum_E"] == want["E"]
    if mode == "per-iteration":
        assert stats["persist_launches"] == 0
    elif mode.startswith("rollcall-fails"):
        # the first resident launch gives up at its roll-call; none is tried after that
        assert stats["persist_launches"] == 1 and stats["persist_aborts"] == 1
    else:
        assert stats["persist_launches"] >= 4 and stats["persist_aborts"] == 0


@pytest.mark.parametrize("seed", list(range(1, 11)))
def test_randomised_streams_whole_batch_resident_launches(seed):
    """Different seeded streams / shapes / workgroup sizes with the engine left to itself (automatic
    threshold: every batch after the first solve is one resident launch, both phases seeded inside
    the kernel): same iterations, frontier sizes and traversed edges as the oracle's synchronous
    schedule, p / r to rounding."""
    rng = np.random.default_rng(1000 + seed)
    scale = int(rng.integers(7, 13))
    edges = int(rng.integers(3000, 40000))
    directed = int(seed % 2)
    W = int(edges * rng.uniform(0.05, 0.3))
    c = int(max(1, W * rng.uniform(0.005, 0.08)))
    eps = float(rng.choice([1e-9, 1e-7, 1e-11]))
    tuning = dict(pull_block=int(rng.choice([256, 512, 1024]))) if seed % 3 else {}
    V, e1, e2 = datagen.rmat_stream(scale, edges, 500 + seed)
    src = int(datagen.top_sources(V, e1, e2, W, directed, 3)[seed % 3])
    sc = Scenario(V, e1, e2, directed, W, c, src, eps, schedule=eng.SCHEDULE_SYNC, **tuning)
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, eps)
    n_batches = 0
    for k in range(7):
        if k:
            if not sc.advance_graphs():
                break
            n_batches += 1
            sc.s.sync_inc_execute(sc.g)
            sc.e.update(sc.slot, eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL, k
    st, want = sc.e.stats(sc.slot), sc.s.stats()
    assert (st["iterations"], st["sum_F"], st["sum_E"]) == (want["iters"], want["F"], want["E"])
    assert st["persist_launches"] >= n_batches and st["persist_aborts"] == 0


@pytest.mark.parametrize("directed", [1, 0])
def test_whole_batch_launch_that_runs_out_of_sweeps_is_resumed(directed):
    """eps = 1e-13 needs ~140 sweeps per batch, more than one resident launch is ever given (128):
    the launch stops mid-phase, the host reads where it stands and resumes -- same work as the
    oracle's synchronous schedule."""
    V, e1, e2 = datagen.rmat_stream(10, 30000, 5)
    W, c, eps = 3000, 60, 1e-13
    src = int(datagen.top_sources(V, e1, e2, W, directed, 1)[0])
    sc = Scenario(V, e1, e2, directed, W, c, src, eps, schedule=eng.SCHEDULE_SYNC)
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, eps)
    it0 = sc.e.stats(sc.slot)["iterations"]
    for k in range(4):
        if k:
            assert sc.advance_graphs()
            sc.s.sync_inc_execute(sc.g)
            sc.e.update(sc.slot, eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL
    st, want = sc.e.stats(sc.slot), sc.s.stats()
    assert (st["iterations"], st["sum_F"], st["sum_E"]) == (want["iters"], want["F"], want["E"])
    # every batch needed more iterations than its launch could run (and one step for the phase switch)
    assert (st["iterations"] - it0) / 3 > 128 and st["persist_launches"] >= 3 and st["persist_aborts"] == 0


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_randomised_streams_sync_frontiers(seed):
    """Different seeded streams / shapes, each with the path thresholds lowered in a different way:
    per-iteration frontier sets must equal the oracle's synchronous schedule on every one."""
    rng = np.random.default_rng(seed)
    scale = int(rng.integers(7, 12))
    edges = int(rng.integers(2000, 12000))
    directed = int(seed % 2)
    W = int(edges * rng.uniform(0.05, 0.3))
    c = int(max(1, W * rng.uniform(0.005, 0.08)))
    tuning = dict(hub_min_degree=int(rng.integers(1, 6)), big_row_edges=int(rng.integers(1, 12)),
                  pull_min_frontier=int(rng.choice([-1, 1, 8, 64])), chunk_iters=int(rng.choice([1, 2, 5, 24])),
                  pull_block=int(rng.choice([256, 384, 576, 640, 896, 1024])))
    V, e1, e2 = datagen.rmat_stream(scale, edges, 100 + seed)
    src = int(datagen.top_sources(V, e1, e2, W, directed, 3)[seed % 3])
    eps = float(rng.choice([1e-9, 1e-7]))
    sc = Scenario(V, e1, e2, directed, W, c, src, eps, schedule=eng.SCHEDULE_SYNC, **tuning)
    sc.s.trace(True)
    sc.e.trace_enable(sc.slot, True)
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, eps)
    for k in range(4):
        if k:
            if not sc.advance_graphs():
                break
            sc.s.trace(True)
            sc.e.trace_enable(sc.slot, True)
            sc.s.sync_inc_execute(sc.g)
            sc.e.update(sc.slot, eps)
        want, got = sc.s.traced_frontiers(), sc.e.trace_get(sc.slot)
        assert len(want) == len(got), (tuning, k)
        for a, b in zip(got, want):
            assert np.array_equal(np.sort(a), np.sort(b)), (tuning, k)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL * max(1.0, eps / 1e-9) and np.max(np.abs(r)) < eps


def test_hub_table_overflow_and_long_row_list_overflow():
    """More candidate hubs than the 2048-slot table (threshold selection kicks in) and more long
    rows per sweep group than the 64-entry workgroup list (owning wave keeps the rest)."""
    V, e1, e2 = datagen.rmat_stream(13, 60000, 21)
    W, c, eps = 30000, 300, 1e-9
    src = int(datagen.top_sources(V, e1, e2, W, 0, 1)[0])
    for tuning in (dict(hub_min_degree=1, big_row_edges=1, pull_min_frontier=-1),   # all hubs, all big (push)
                   dict(hub_min_degree=1, big_row_edges=1, pull_min_frontier=1)):   # every row "long" (pull)
        sc = Scenario(V, e1, e2, 0, W, c, src, eps, schedule=eng.SCHEDULE_SYNC, **tuning)
        sc.s.sync_execute(sc.g)
        sc.e.init_solve(sc.slot, eps)
        for k in range(3):
            if k:
                assert sc.advance_graphs()
                sc.s.sync_inc_execute(sc.g)
                sc.e.update(sc.slot, eps)
            p, r = sc.e.read(sc.slot)
            assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL
            st, want = sc.e.stats(sc.slot), sc.s.stats()
            assert (st["iterations"], st["sum_F"], st["sum_E"]) == (want["iters"], want["F"], want["E"])


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_randomised_streams_eager_production_mode(seed):
    """Production (eager) schedule on random shapes / thresholds, chunked launches, no trace:
    north-star tolerance vs the cpu/PPRCPUMTCilkRev restatement, Validate() criteria, invariant."""
    rng = np.random.default_rng(seed)
    scale = int(rng.integers(8, 13))
    edges = int(rng.integers(3000, 30000))
    directed = int(seed % 2)
    W = int(edges * rng.uniform(0.05, 0.3))
    c = int(max(1, W * rng.uniform(0.005, 0.05)))
    tuning = dict(hub_min_degree=int(rng.integers(1, 8)), big_row_edges=int(rng.integers(1, 40)),
                  pull_min_frontier=int(rng.choice([-1, 1, 16, 0])), chunk_iters=int(rng.choice([1, 3, 24])),
                  pull_block=int(rng.choice([0, 256, 512, 768])))
    V, e1, e2 = datagen.rmat_stream(scale, edges, 200 + seed)
    src = int(datagen.top_sources(V, e1, e2, W, directed, 2)[seed % 2])
    eps = 1e-9
    sc = Scenario(V, e1, e2, directed, W, c, src, eps, **tuning)
    sc.s.cilk_execute(sc.g)
    sc.e.init_solve(sc.slot, eps)
    for k in range(6):
        if k:
            if not sc.advance_graphs():
                break
            sc.s.cilk_inc_execute(sc.g)
            sc.e.update(sc.slot, eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(r)) < eps, (tuning, k)
        assert np.max(np.abs(p - sc.s.p)) < NORTH_STAR_TOL, (tuning, k)
        pw, _ = orc.pow_rev(sc.g, sc.source)
        assert np.max(np.abs(p - pw)) < 100 * eps
        s_, d_ = window_directed_edges(sc.g)
        assert invariant_max_err_np(p, r, s_, d_, sc.V, sc.source) < INVARIANT_TOL


@pytest.mark.parametrize("directed", [1, 0])
def test_incremental_graph_equals_full_rebuild(directed):
    """f1: merging each batch into the previous sorted keys gives the same device CSRs (in, out,
    degrees) as re-sorting the whole window -- duplicate edges, ring wrap-around and a batch larger
    than half the window (falls back to the full sort) included."""
    rng = np.random.default_rng(9)
    V, n = 40, 3000
    e1 = rng.integers(0, V, n).astype(np.int32)          # tiny id range: many duplicate edges, self loops
    e2 = rng.integers(0, V, n).astype(np.int32)
    for W, c in ((300, 7), (300, 100), (64, 40)):
        a = Scenario(V, e1, e2, directed, W, c, 1, 1e-9)
        b = Scenario(V, e1, e2, directed, W, c, 1, 1e-9)
        b.e.set_incremental_graph(False)
        for _ in range(12):
            assert a.advance_graphs() and b.advance_graphs()
            check_csr(a)
            ra, ca, da = a.e.read_graph()
            rb, cb, db = b.e.read_graph()
            assert np.array_equal(ra, rb) and np.array_equal(ca, cb) and np.array_equal(da, db)
            oa, ob = a.e.read_out_graph(), b.e.read_out_graph()
            assert np.array_equal(oa[0], ob[0]) and np.array_equal(oa[1], ob[1])


@pytest.mark.parametrize("tuning", VARIANT_TUNINGS, ids=VARIANT_IDS)
@pytest.mark.parametrize("directed", [1, 0])
def test_eager_variant_with_status_array_filter(directed, tuning):
    """dppr_set_variant(2 EAGER): eager residual reads, next frontier through the status array
    (legal(curr) && atomicExch(status[v], level) < level, gpu/ExpandRev.cuh:255,298,340) instead of the crossing test. Against
    the oracle's restatement of PPRCPUMTCilkRevEager and of the default variant (bit-identical to each other at -t 1) within the
    north-star tolerance, plus the reference's Validate() criteria."""
    eps = 1e-9
    sc = make(directed, c=30, eps=eps, tuning=dict(tuning, variant=2))
    v2 = orc.State(sc.V, sc.source, eps)
    sc.s.cilk_execute(sc.g)
    v2.variant_execute(sc.g, 2)
    sc.e.init_solve(sc.slot, eps)
    for k in range(6):
        if k:
            assert sc.advance_graphs()
            sc.s.cilk_inc_execute(sc.g)
            v2.variant_inc_execute(sc.g, 2)
            sc.e.update(sc.slot, eps)
        p, r = sc.e.read(sc.slot)
        assert np.array_equal(v2.p, sc.s.p)                       # the reference's variants 0 and 2 are one schedule
        assert np.max(np.abs(r)) < eps and np.max(np.abs(p - v2.p)) < NORTH_STAR_TOL
        src, dst = window_directed_edges(sc.g)
        assert invariant_max_err_np(p, r, src, dst, sc.V, sc.source) < INVARIANT_TOL


MERGE_TUNINGS = [dict(pull_min_frontier=-1), dict(hub_min_degree=3, big_row_edges=8, pull_min_frontier=-1), dict(pull_min_frontier=1, persistent=0),
                 dict(pull_min_frontier=1), dict(pull_min_frontier=40, chunk_iters=3), dict(pull_min_frontier=1, pull_block=256, persist_timeout_us=-1),
                 dict(pull_min_frontier=1, persistent=0, binned=(2, 1, 1, 64, 0, 64, 64)), dict(pull_min_frontier=1, persistent=0, sweep_bitmap=1, pull_block=256)]
MERGE_IDS = ["push-only", "push-hubs+bigrows", "pull-no-persist", "pull-resident", "mixed-chunk3", "pull-rollcall-fails", "binned", "pull-bitmap"]


@pytest.mark.parametrize("tuning", MERGE_TUNINGS, ids=MERGE_IDS)
@pytest.mark.parametrize("directed", [1, 0])
def test_merged_loop_single_source(directed, tuning):
    """dppr_set_phase_merge: residuals of both signs in ONE loop, to eps / 4 (not the reference's schedule; every push is the
    reference's). The state it ends in satisfies the reference's Validate() with room to spare (|r| <= eps / 4), the loop
    invariant to rounding, and p is within the north-star tolerance of cpu/PPRCPUMTCilkRev's result at eps AND of the
    oracle's own merged loop (orc_merged_inc_execute) -- on every launch form."""
    eps, div = 1e-9, 4
    sc = make(directed, c=30, eps=eps, tuning=dict(tuning, merge_phases=div))
    m = orc.State(sc.V, sc.source, eps)
    sc.s.cilk_execute(sc.g)
    m.cilk_execute(sc.g)
    sc.e.init_solve(sc.slot, eps)
    for k in range(6):
        assert sc.advance_graphs()
        sc.s.cilk_inc_execute(sc.g)
        m.merged_inc_execute(sc.g, eps / div)
        sc.e.update(sc.slot, eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(r)) <= eps / div
        assert np.max(np.abs(p - sc.s.p)) < NORTH_STAR_TOL and np.max(np.abs(p - m.p)) < NORTH_STAR_TOL
        pw, _ = orc.pow_rev(sc.g, sc.source)
        assert np.max(np.abs(p - pw)) < 100 * eps                        # gpu/PPRRevPushGPU.cuh:145-156
        src, dst = window_directed_edges(sc.g)
        assert invariant_max_err_np(p, r, src, dst, sc.V, sc.source) < INVARIANT_TOL
    # the split interface still runs the reference's two loops
    assert sc.advance_graphs()
    sc.s.cilk_inc_execute(sc.g)
    sc.e.incremental_batch_update(sc.slot)
    sc.e.execute_main_loop(sc.slot, 0, eps)
    sc.e.execute_main_loop(sc.slot, 1, eps)
    p, r = sc.e.read(sc.slot)
    assert np.max(np.abs(r)) < eps and np.max(np.abs(p - sc.s.p)) < NORTH_STAR_TOL


@pytest.mark.parametrize("tuning", [dict(pull_min_frontier=-1), dict(hub_min_degree=1, big_row_edges=1, pull_min_frontier=-1),
                                    dict(pull_min_frontier=-1, schedule=eng.SCHEDULE_EAGER, variant=2)], ids=["push", "all-hub-all-big", "variant2"])
def test_merged_loop_push_iterations_keep_the_frontier_list_bounded(tuning):
    """A tiny dense window with large batches, every iteration a push iteration: in the merged loop adds of both signs take residuals
    across the threshold again and again inside one iteration. The next frontier holds every vertex at most once (status-array
    filter; with the crossing test alone each crossing would append and the V-entry list could overflow): 40 batches against the
    oracles, the state intact throughout."""
    V, W, c, eps, div = 64, 600, 150, 1e-9, 4
    rng = np.random.default_rng(23)
    n = W + 41 * c
    e1 = rng.integers(0, V, n).astype(np.int32)
    e2 = rng.integers(0, V, n).astype(np.int32)
    e2 = np.where(e2 == e1, (e2 + 1) % V, e2).astype(np.int32)
    sc = Scenario(V, e1, e2, 1, W, c, 5, eps, **dict(tuning, merge_phases=div))
    m = orc.State(V, 5, eps)
    sc.s.cilk_execute(sc.g)
    m.cilk_execute(sc.g)
    sc.e.init_solve(sc.slot, eps)
    for k in range(40):
        assert sc.advance_graphs()
        sc.s.cilk_inc_execute(sc.g)
        m.merged_inc_execute(sc.g, eps / div)
        sc.e.update(sc.slot, eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(r)) <= eps / div and np.max(np.abs(p - sc.s.p)) < NORTH_STAR_TOL and np.max(np.abs(p - m.p)) < NORTH_STAR_TOL, k
        src, dst = window_directed_edges(sc.g)
        assert invariant_max_err_np(p, r, src, dst, V, 5) < INVARIANT_TOL
    check_csr(sc)


@pytest.mark.parametrize("mode", ["sweeps", "push-tail", "multi-sweep"])
@pytest.mark.parametrize("nsrc,directed", [(3, 1), (10, 0), (16, 1)])
def test_merged_loop_source_group(nsrc, directed, mode):
    """The merged loop of a source group is a synchronous schedule like its two loops: per source it equals the oracle's merged
    loop (orc_merged_inc_execute at eps / 4) to the rounding of the sums, with the same frontier and edge totals; and it is within
    the north-star tolerance of cpu/PPRCPUMTCilkRev at eps."""
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    W, c, eps, div = 600, 25, 1e-9, 4
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, nsrc)]
    e = eng.Engine(V, W, directed, c, merge_phases=div, **(dict(chunk_iters=3) if mode == "multi-sweep" else {}))
    e.set_group_resident(mode == "multi-sweep")
    e.set_group_push(*((40, 0, 0) if mode == "push-tail" else (0, 0, 0)))
    g = orc.Graph(V, e1, e2, directed, W, c)
    merged = [orc.State(V, s, eps) for s in sources]
    cilk = [orc.State(V, s, eps) for s in sources]
    e.load_window(*g.window_edges())
    gid = e.add_source_group(sources)
    for s in merged + cilk:
        s.sync_execute(g)
    e.group_init_solve(gid, eps)
    for s in merged:
        s.reset_stats()
    e.group_reset_stats(gid)
    for k in range(5):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        for s in merged:
            s.merged_inc_execute(g, eps / div)
        for s in cilk:
            s.cilk_inc_execute(g)
        e.group_update(gid, eps)
        for i in range(nsrc):
            p, r = e.group_read(gid, i)
            assert np.max(np.abs(p - merged[i].p)) < SYNC_TOL and np.max(np.abs(r - merged[i].r)) < SYNC_TOL, (k, i)
            assert np.max(np.abs(r)) <= eps / div and np.max(np.abs(p - cilk[i].p)) < NORTH_STAR_TOL
    st = e.group_stats(gid)
    assert st["sum_F"] == sum(s.stats()["F"] for s in merged) and st["sum_E"] == sum(s.stats()["E"] for s in merged)
    e.close()


def run_source_group(V, e1, e2, W, c, eps, directed, sources, batches, seeding, tuning=None, resident=True, push=None):
    """Drive a source group and one oracle state per source (synchronous schedule) over the same
    stream; per-source p/r to rounding, summed statistics equal."""
    e = eng.Engine(V, W, directed, c, **(tuning or {}))
    e.set_group_seeding(seeding == "tails")
    e.set_group_resident(resident)
    if push is not None:
        e.set_group_push(*push)
    g = orc.Graph(V, e1, e2, directed, W, c)
    states = [orc.State(V, s, eps) for s in sources]
    e.load_window(*g.window_edges())
    gid = e.add_source_group(sources)
    for s in states:
        s.sync_execute(g)
    e.group_init_solve(gid, eps)
    inspected0 = e.group_stats(gid)["inspected"]
    for k in range(batches + 1):
        if k:
            assert not g.stream_updates()
            g.inc_construct(1)
            e.set_batch(*g.batch())
            e.slide(*g.new_stream())
            for s in states:
                s.sync_inc_execute(g)
            e.group_update(gid, eps)
        for i, s in enumerate(states):
            p, r = e.group_read(gid, i)
            assert np.max(np.abs(p - s.p)) < SYNC_TOL and np.max(np.abs(r - s.r)) < SYNC_TOL, (k, i)
    st = e.group_stats(gid)
    assert st["sum_F"] == sum(s.stats()["F"] for s in states)
    assert st["sum_E"] == sum(s.stats()["E"] for s in states)
    assert st["iterations"] <= sum(s.stats()["iters"] for s in states)
    # dense seeding scans every vertex twice per batch, tail seeding none after the from-scratch solve
    assert inspected0 > 0 and ((st["inspected"] > inspected0) if seeding == "dense" else (st["inspected"] == inspected0))
    return e, gid


@pytest.mark.parametrize("seeding", ["tails", "dense"])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 5, 6, 8, 9, 10, 11, 12, 13, 16])
@pytest.mark.parametrize("directed", [1, 0])
def test_source_group_matches_oracle_per_source(directed, nsrc, seeding):
    """f2: up to 16 sources solved together on interleaved state (rows of 2 * ceil(n / 2) doubles: every
    row width from 2 to 16 is exercised, with and without a padding double). Every source's p/r must equal the oracle's synchronous schedule for that source (group
    iterations are sweeps), and the summed statistics must equal the sum of the per-source oracle
    runs -- with the frontier seeded from the batch tails and with full Inspect passes."""
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    W, c, eps = 600, 20, 1e-9
    sources = [int(s) for s in datagen.top_sources(V, e1, e2, W, directed, nsrc)]
    e, gid = run_source_group(V, e1, e2, W, c, eps, directed, sources, 5, seeding)
    with pytest.raises(eng.DpprError):
        e.add_source_group(list(range(17)))
    with pytest.raises(eng.DpprError):
        e.group_read(gid, nsrc)


@pytest.mark.parametrize("shape", ["many-groups-hubs", "one-hub-row-spans-all-octets", "tiny-window"])
@pytest.mark.parametrize("nsrc", [5, 9, 10, 12])
def test_source_group_sweep_shapes(nsrc, shape):
    """k_gsweep splits a sweep group's edges evenly over its 128 octets: windows with several
    sweep groups and hub rows, a window in which one row holds most edges (every octet walks a
    piece of the same row), and a window smaller than one step per octet."""
    rng = np.random.default_rng(17)
    if shape == "many-groups-hubs":
        V, e1, e2 = datagen.rmat_stream(13, 60000, 21)
        W, c, directed = 30000, 300, 0
    elif shape == "one-hub-row-spans-all-octets":
        V, n = 3000, 40000
        e1 = np.where(rng.random(n) < 0.8, 7, rng.integers(0, V, n)).astype(np.int32)   # 80 % of the edges leave vertex 7
        e2 = rng.integers(0, V, n).astype(np.int32)
        e2 = np.where(e2 == e1, (e2 + 1) % V, e2).astype(np.int32)
        W, c, directed = 20000, 200, 1
    else:
        V, e1, e2 = datagen.rmat_stream(6, 900, 3)
        W, c, directed = 40, 3, 1
    ranked = datagen.top_sources(V, e1, e2, W, directed, 40)
    sources = [int(s) for s in ranked[::4][:nsrc]]
    run_source_group(V, e1, e2, W, c, 1e-9, directed, sources, 4, "tails")


@pytest.mark.parametrize("mode", ["one-launch-per-sweep", "multi-sweep", "multi-sweep-3-at-a-time", "rollcall-fails"])
@pytest.mark.parametrize("nsrc", [4, 10, 11, 12])
def test_source_group_launch_forms(nsrc, mode):
    """The frontier loop of a source group as one launch per sweep, as multi-sweep launches (grid barrier
    between sweeps; the default on windows whose groups are all resident), as multi-sweep launches that
    may only run 3 sweeps and are resumed, and with a roll-call that cannot succeed (the launch gives up
    untouched, one-sweep launches go on): same per-source results and statistics."""
    V, e1, e2 = datagen.rmat_stream(12, 40000, 7)
    W, c, directed = 12000, 120, 0
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, nsrc)]
    tuning = {"multi-sweep-3-at-a-time": dict(chunk_iters=3), "rollcall-fails": dict(persist_timeout_us=-1)}.get(mode)
    e, gid = run_source_group(V, e1, e2, W, c, 1e-9, directed, sources, 3, "tails", tuning=tuning,
                              resident=mode != "one-launch-per-sweep")
    st = e.group_stats(gid)
    if mode == "one-launch-per-sweep":
        assert st["persist_launches"] == 0
    elif mode == "rollcall-fails":
        assert st["persist_launches"] == 1 and st["persist_aborts"] == 1
    else:
        assert st["persist_launches"] >= 7 and st["persist_aborts"] == 0
        if mode == "multi-sweep-3-at-a-time":
            assert st["persist_launches"] > st["iterations"] / 4


@pytest.mark.parametrize("mode", ["automatic", "never", "as-early-as-possible", "as-early-as-possible-chunk2", "tiny-lists", "below-50-pairs",
                                  "iterations-call-themselves-off"])
@pytest.mark.parametrize("seeding", ["tails", "dense"])
@pytest.mark.parametrize("nsrc,directed", [(3, 1), (6, 0), (9, 1), (10, 0), (11, 1), (12, 0), (16, 1)])
def test_source_group_tail_as_pushes(nsrc, directed, seeding, mode):
    """The tail of a group's loop in push form (dppr_gpush.hpp), one-sweep launches before it: entered at the automatic
    threshold, never, at every chunk boundary (iterations too large for the form call themselves off and the loop goes
    back to sweeps, to try again on a much smaller frontier -- forced with a bound of 3000 in-edges per iteration),
    with frontier lists of 1024 vertices (longer frontiers do not enter), below 50 pairs. Per-source p / r, sum F and sum E of the oracle's synchronous schedule every time."""
    V, e1, e2 = datagen.rmat_stream(13, 70000, 21)
    W, c = 20000, 200
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, nsrc)]
    push = {"automatic": (-1, 0), "never": (0, 0), "as-early-as-possible": (10**9, 0), "as-early-as-possible-chunk2": (10**9, 0),
            "tiny-lists": (10**9, 1024), "below-50-pairs": (50, 0), "iterations-call-themselves-off": (10**9, 0, 3000)}[mode]
    tuning = dict(chunk_iters=2) if mode.endswith("chunk2") or mode.endswith("off") else None
    e, gid = run_source_group(V, e1, e2, W, c, 1e-9, directed, sources, 4, seeding, tuning=tuning, resident=False, push=push)
    st = e.group_stats(gid)
    assert st["persist_launches"] == 0
    if mode == "never":
        assert st["pull_iterations"] == st["iterations"]
    elif mode != "tiny-lists":  # (there a frontier that does not fit the lists simply stays with the sweeps)
        assert st["pull_iterations"] < st["iterations"]  # some iterations ran as pushes


PROFILED_FORMS = {
    # single source, one launch per iteration
    "pushes": dict(pull_min_frontier=-1, persistent=0),
    "gather-sweeps": dict(pull_min_frontier=1, persistent=0),
    "bitmap-sweeps": dict(pull_min_frontier=1, persistent=0, sweep_bitmap=1, pull_block=256),
    "binned-sweeps": dict(pull_min_frontier=1, persistent=0, binned=(2, 1, 1, 64, 0, 64, 64)),
    # single source, resident launches (the default), and with a roll-call that cannot succeed
    "resident": dict(pull_min_frontier=1),
    "resident-rollcall-fails": dict(pull_min_frontier=1, persist_timeout_us=-1),
    # a source group of 10 without a push tail: one launch per sweep, multi-sweep launches
    "group-one-launch-per-sweep": None,
    "group-multi-sweep": None,
}


def _profiled_stats(form, profiling):
    """Statistics of a from-scratch solve and four batches of the toy stream on one launch form."""
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    W, c, eps, directed = 600, 20, 1e-9, 1
    g = orc.Graph(V, e1, e2, directed, W, c)
    group = form.startswith("group-")
    e = eng.Engine(V, W, directed, c, schedule=eng.SCHEDULE_SYNC, **(PROFILED_FORMS[form] or {}))
    e.set_profiling(profiling)
    e.load_window(*g.window_edges())
    if group:
        e.set_group_resident(form == "group-multi-sweep")
        e.set_group_push(0, 0, 0)
        h = e.add_source_group([int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 10)])
        e.group_init_solve(h, eps)
    else:
        h = e.add_source(int(datagen.top_sources(V, e1, e2, W, directed, 1)[0]))
        e.init_solve(h, eps)
    for _ in range(4):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        if group:
            e.group_update(h, eps)
        else:
            e.update(h, eps)
    st = e.group_stats(h) if group else e.stats(h)
    e.close()
    return st


@pytest.mark.parametrize("form", list(PROFILED_FORMS))
def test_profiling_counters_of_every_launch_form(form):
    """dppr_set_profiling: push_ms / push_launches count every timed launch of a loop, sweep_ms / sweep_launches those of them
    that were ONE sweep. A launch per iteration: one timed launch per iteration that saw a frontier, the sweeps among them
    counted twice. Resident and multi-sweep launches: one timed launch each unless the roll-call failed, and none of them is a
    sweep launch; after a failed roll-call the loops go on one launch per iteration. Without profiling the four words stay 0."""
    off = _profiled_stats(form, False)
    assert (off["push_launches"], off["sweep_launches"], off["push_ms"], off["sweep_ms"]) == (0, 0, 0.0, 0.0)
    st = _profiled_stats(form, True)
    print({k: st[k] for k in ("iterations", "pull_iterations", "push_launches", "sweep_launches", "persist_launches", "persist_aborts",
                              "binned_sweeps", "push_ms", "sweep_ms")})
    assert st["iterations"] > 0 and st["push_launches"] > 0 and st["push_ms"] > 0
    for k in ("iterations", "pull_iterations", "persist_launches", "persist_aborts", "binned_sweeps", "sum_F"):
        assert st[k] == off[k], k   # (profiling changes no launch)
    per_iteration = form in ("pushes", "gather-sweeps", "bitmap-sweeps", "binned-sweeps", "resident-rollcall-fails",
                             "group-one-launch-per-sweep")
    if form == "resident-rollcall-fails":   # the first resident launch gave up untouched, none was tried after it
        assert st["persist_aborts"] >= 1 and st["persist_launches"] == st["persist_aborts"]
    elif per_iteration:
        assert st["persist_launches"] == 0
    if per_iteration:
        assert st["push_launches"] == st["iterations"] and st["sweep_launches"] == st["pull_iterations"]
        assert (st["pull_iterations"] == 0) == (form == "pushes")
        if st["sweep_launches"]:
            assert 0 < st["sweep_ms"] <= st["push_ms"]
        else:
            assert st["sweep_ms"] == 0
        assert st["binned_sweeps"] == (st["sweep_launches"] if form == "binned-sweeps" else 0)
        if form.startswith("group-"):
            assert st["sweep_launches"] == st["iterations"]
    else:   # resident / multi-sweep launches
        assert st["persist_launches"] > st["persist_aborts"]
        assert st["push_launches"] == st["persist_launches"] - st["persist_aborts"]
        assert st["sweep_launches"] == 0 and st["sweep_ms"] == 0


def test_source_group_sources_outside_the_window_and_duplicates():
    """Sources that have no edge in the window (fresh internal ids: the sweep groups are re-cut) and
    the same vertex twice in one group."""
    V, e1, e2 = datagen.rmat_stream(10, 8000, 9)
    W, c, directed = 500, 10, 1
    used = set(e1[:W + 60 * c].tolist()) | set(e2[:W + 60 * c].tolist())
    lonely = [v for v in range(V) if v not in used][:2]
    top = [int(s) for s in datagen.top_sources(V, e1, e2, W, directed, 2)]
    run_source_group(V, e1, e2, W, c, 1e-9, directed, lonely + top + [top[0]], 4, "tails")


def test_binned_tables_that_cannot_be_allocated_fall_back_to_gather_sweeps(monkeypatch):
    """the binned-sweep tables are an optimisation. When their allocations fail (test hook
    DPPR_TEST_BIN_OOM: every one of them reports out-of-memory) dppr_load_window / dppr_slide / dppr_add_source still
    succeed, the sweeps gather (k_pull_iter) and the results are the oracle's; once memory is there again the next epoch gets
    its tables."""
    monkeypatch.setenv("DPPR_TEST_BIN_OOM", "1")
    sc = make(1, schedule=eng.SCHEDULE_SYNC, scale=12, edges=60000, seed=5, W=20000, c=200,
              tuning=dict(binned=(2, 0, 0, 0, 0), pull_min_frontier=1, persistent=0))
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)
    for k in range(3):
        if k == 2:
            monkeypatch.delenv("DPPR_TEST_BIN_OOM")   # (the slide of this batch can allocate again)
        assert sc.advance_graphs()
        sc.s.sync_inc_execute(sc.g)
        sc.e.update(sc.slot, sc.eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL
        st = sc.e.stats(sc.slot)
        assert st["pull_iterations"] > 0
        assert (st["binned_sweeps"] == 0) if k < 2 else (st["binned_sweeps"] > 0), (k, st["binned_sweeps"])


@pytest.mark.parametrize("shape", [(2, 1, 1, 64, 0, 64, 64), (2, 2, 3, 200, 0, 100, 500), (2, 0, 0, 0, 0)])
@pytest.mark.parametrize("directed", [1, 0])
def test_binned_tables_placed_by_counting_equal_the_sorted_ones(monkeypatch, directed, shape):
    """The B-major order of the binned tables by k_bin_bmajor (a histogram + one ordered walk per B-block; chosen by itself only
    where the radix sort would need four passes: friendster-size windows) forced on small windows (DPPR_BIN_PLACEMENT=counting):
    dozens of tiny blocks, blocks of a few tiles -- hub rows alone in their block, which are copied --, and one block for
    everything. The same stable order as the sort, so the sweeps do the oracle's work exactly and give its p / r to rounding."""
    monkeypatch.setenv("DPPR_BIN_PLACEMENT", "counting")
    sc = make(directed, schedule=eng.SCHEDULE_SYNC, scale=12, edges=60000, seed=5, W=20000, c=200,
              tuning=dict(binned=shape, pull_min_frontier=1, persistent=0))
    sc.s.sync_execute(sc.g)
    sc.e.init_solve(sc.slot, sc.eps)
    for k in range(4):
        assert sc.advance_graphs()
        sc.s.sync_inc_execute(sc.g)
        sc.e.update(sc.slot, sc.eps)
        p, r = sc.e.read(sc.slot)
        assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL, k
    st, w = sc.e.stats(sc.slot), sc.s.stats()
    assert (st["iterations"], st["sum_F"], st["sum_E"]) == (w["iters"], w["F"], w["E"]) and st["binned_sweeps"] == st["pull_iterations"] > 0
    sc.e.close()


@pytest.mark.parametrize("directed", [1, 0])
def test_lookahead_id_lookups_change_nothing(directed):
    """dppr_hint_next_batch: the next batch's id arrays announced before the update, looked up on helper
    threads while it runs, consumed by set_batch / slide -- with ids that have no internal id yet (fresh vertices arrive with most
    batches of this stream) and, with renumbering forced at every slide, with hints that a renumbering invalidates. The device
    CSR stays the oracle's every slide, p / r the synchronous oracle's, and the hint is actually used (dppr_debug_dump counts it)."""
    for forced in (False, True):
        sc = make(directed, schedule=eng.SCHEDULE_SYNC, scale=11, edges=30000, seed=17, W=3000, c=60)
        if forced:
            sc.e.set_renumbering(1, growth_pct=1, min_parked=1)
        sc.s.sync_execute(sc.g)
        sc.e.init_solve(sc.slot, sc.eps)
        assert not sc.g.stream_updates()
        sc.g.inc_construct(1)
        nxt = (*sc.g.batch()[:2], *sc.g.new_stream())          # batch 1: no hint (nothing ran before it)
        ins = sc.g.batch()[2]
        for k in range(8):
            sc.e.set_batch(nxt[0], nxt[1], ins)
            sc.e.slide(nxt[2], nxt[3])
            check_csr(sc)
            sc.s.sync_inc_execute(sc.g)
            more = not sc.g.stream_updates()                   # the host stream moves on to batch k + 2 BEFORE the update ...
            if more:
                sc.g.inc_construct(1)
                b1, b2, ins = sc.g.batch()
                n1, n2 = sc.g.new_stream()
                if k % 2:                                      # ... whose id lookups run while it does
                    nxt = sc.e.hint_next_batch(b1, b2, n1, n2)
                else:                                          # (hinted from a helper thread DURING the update, as ./pagerank does)
                    box = []
                    th = threading.Thread(target=lambda: box.append(sc.e.hint_next_batch(b1, b2, n1, n2)))
                    th.start()
            sc.e.update(sc.slot, sc.eps)
            if more and not k % 2:
                th.join()
                nxt = box[0]
            p, r = sc.e.read(sc.slot)
            assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL, (forced, k)
            if not more:
                break
        text = sc.e.debug_dump()
        hits = int(text.split("id lookahead (dppr_hint_next_batch): ")[1].split(" ")[0])
        assert hits >= (4 if not forced else 2), text   # (a renumbering slide drops the hint for its own two arrays, never the batch's)
        sc.e.close()


def test_a_hint_whose_buffers_were_refilled_is_dropped():
    """the lookahead is matched by pointer and length; a caller that refills the announced buffers with ANOTHER batch
    before handing them over must get that batch's edges, not the announced ones (content samples are checked before a hint is
    trusted). Device CSR == oracle after every slide."""
    sc = make(1, scale=11, edges=30000, seed=23, W=3000, c=60)
    sc.e.init_solve(sc.slot, sc.eps)
    for k in range(4):
        assert not sc.g.stream_updates()
        sc.g.inc_construct(1)
        b1, b2, ins = sc.g.batch()
        n1, n2 = sc.g.new_stream()
        # announce buffers of the right shape but with OTHER ids, then overwrite them in place with the real batch
        h = sc.e.hint_next_batch(np.roll(b1, 1), np.roll(b2, 3), np.roll(n1, 2), np.roll(n2, 5))
        time.sleep(0.05)                                    # (the helper's lookups of a few hundred ids are long over)
        for dst, src in zip(h, (b1, b2, n1, n2)):
            dst[:] = src
        sc.e.set_batch(h[0], h[1], ins)
        sc.e.slide(h[2], h[3])
        check_csr(sc)
        sc.e.update(sc.slot, sc.eps)
    sc.e.close()


def test_a_slide_whose_key_merge_misses_a_key_resorts_the_window(monkeypatch):
    """k_del_positions counts the retired keys it cannot find in the kept sorted keys; a slide that finds one discards
    the merge and re-sorts the whole window (test hook DPPR_TEST_MERGE_MISS: every incremental slide takes that path). The device
    CSR stays the oracle's."""
    monkeypatch.setenv("DPPR_TEST_MERGE_MISS", "1")
    sc = make(0, W=100, c=7, edges=2000)
    for _ in range(10):
        assert sc.advance_graphs()
        check_csr(sc)
    text = sc.e.debug_dump()
    assert "re-sorted the window (a retired key was missing): 10" in text, text
    sc.e.close()


def test_debug_dump_reads_the_engine_from_another_thread():
    """dppr_debug_dump (the hang post-mortem): host-side loop state plus the device words, read through a side stream;
    also after a launch whose roll-call cannot succeed (persist_timeout_us = -1: the launch gives up untouched)."""
    sc = make(0, c=20, tuning=dict(persist_timeout_us=-1))
    sc.e.init_solve(sc.slot, sc.eps)
    for _ in range(2):
        assert sc.advance_graphs()
        sc.e.update(sc.slot, sc.eps)
    text = sc.e.debug_dump()
    assert "last error: (none)" in text and "engine stream: idle" in text
    assert "GridBar: gen" in text and "slot 0: source" in text
    assert sc.e.stats(sc.slot)["persist_aborts"] >= 1 and "ok 0" in text   # the failed roll-call switched resident launches off
    assert sc.e.time_batch_grouping(reps=3) > 0.0


def test_two_engines_on_one_device_from_two_threads():
    """Two engines share device 0 and are driven from two host threads at once: their resident
    launches compete for the same CUs (each wants all of them). Whatever the interleaving -- one
    waits for the other, or a roll-call gives up and that engine goes on with per-iteration
    launches -- both must finish and match the oracle."""
    import threading
    V, e1, e2 = datagen.rmat_stream(12, 60000, 31)
    W, c, eps = 6000, 60, 1e-9
    srcs = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 2)]
    scs = [Scenario(V, e1, e2, 0, W, c, s_, eps, schedule=eng.SCHEDULE_SYNC, pull_min_frontier=1) for s_ in srcs]
    errors = []

    def drive(sc):
        try:
            sc.s.sync_execute(sc.g)
            sc.e.init_solve(sc.slot, eps)
            for _ in range(12):
                assert sc.advance_graphs()
                sc.s.sync_inc_execute(sc.g)
                sc.e.update(sc.slot, eps)
                p, r = sc.e.read(sc.slot)
                assert np.max(np.abs(p - sc.s.p)) < SYNC_TOL and np.max(np.abs(r - sc.s.r)) < SYNC_TOL
        except BaseException as ex:  # noqa: BLE001 - reported by the main thread
            errors.append(repr(ex))

    threads = [threading.Thread(target=drive, args=(sc,), daemon=True) for sc in scs]
    for t in threads:
        t.start()
    deadline = time.monotonic() + 90
    for t in threads:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):   # post-mortem into the pytest log: Python stacks + both engines' device-side state
        import faulthandler
        faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
        pytest.fail("a driver thread hangs; engine state:\n" + "\n".join(sc.e.debug_dump() for sc in scs))
    assert not errors, errors
    assert sum(sc.e.stats(sc.slot)["persist_launches"] for sc in scs) > 0


def test_narrow_and_wide_source_groups_share_an_engine():
    """An 8-wide and a 16-wide group on ONE engine: the epochs' group tables are then cut for 512-vertex
    groups and the 8-wide sweep runs on them too (k_gsweep<1, 512>); results per source as always."""
    V, e1, e2 = datagen.rmat_stream(11, 30000, 13)
    W, c, directed, eps = 6000, 60, 1, 1e-9
    top = [int(x) for x in datagen.top_sources(V, e1, e2, W, directed, 14)]
    narrow, wide = top[:4], top[4:]
    e = eng.Engine(V, W, directed, c, n_epochs=4)
    g = orc.Graph(V, e1, e2, directed, W, c)
    states = [orc.State(V, s, eps) for s in narrow + wide]
    e.load_window(*g.window_edges())
    ga = e.add_source_group(narrow)
    e.group_init_solve(ga, eps)                   # solved on 1024-vertex tables ...
    gb = e.add_source_group(wide)                  # ... which are re-cut for 512 here
    e.group_init_solve(gb, eps)
    for s in states:
        s.sync_execute(g)
    for k in range(1, 4):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        for s in states:
            s.sync_inc_execute(g)
        e.group_update(ga, eps, epoch=k)
        e.group_update(gb, eps, epoch=k)
        for i, s in enumerate(states):
            p, r = e.group_read(ga, i) if i < 4 else e.group_read(gb, i - 4)
            assert np.max(np.abs(p - s.p)) < SYNC_TOL and np.max(np.abs(r - s.r)) < SYNC_TOL, (k, i)
