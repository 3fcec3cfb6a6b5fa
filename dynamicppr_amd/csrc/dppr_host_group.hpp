// dppr_host_group.hpp -- host side, part 4 of 4: source groups (f2). The frontier loop of up to 16 sources solved together:
// one-sweep and multi-sweep launches of k_gsweep, the push form of a loop's tail (dppr_gpush.hpp), the group's stream update,
// and the sequence of one batch (group_update).
#pragma once

namespace {

// ---------------------------------------------------------------------------- f2: groups
// The group kernels are instantiated per row width (dppr_multi.hpp: GW = 2, 4, .. 16 doubles; one double per lane of
// an octet up to 8, two beyond), the sweep also per size of a sweep group (nvx vertices: 1024, or 512 once a 16-wide group
// exists -- a wide row always, a narrow one on an engine that also has a wide group): f(SPL, GW, NVX) is called with the
// three as compile-time constants.
template <class F>
void with_row(int gw, int nvx, F &&f) {
    auto narrow = [&](auto w) {
        if (nvx == 512) f(IC<1>{}, w, IC<512>{});
        else f(IC<1>{}, w, IC<1024>{});
    };
    switch (gw) {
    case 2: narrow(IC<2>{}); break;
    case 4: narrow(IC<4>{}); break;
    case 6: narrow(IC<6>{}); break;
    case 8: narrow(IC<8>{}); break;
    case 10: f(IC<2>{}, IC<10>{}, IC<512>{}); break;
    case 12: f(IC<2>{}, IC<12>{}, IC<512>{}); break;
    case 14: f(IC<2>{}, IC<14>{}, IC<512>{}); break;
    default: f(IC<2>{}, IC<16>{}, IC<512>{}); break;
    }
}
template <class F>
void with_row(int gw, F &&f) { // (kernels that do not depend on the sweep groups: f(SPL, GW))
    with_row(gw, 512, [&](auto spl, auto w, auto) { f(spl, w); });
}

// One launch of k_gsweep (dppr_multi.hpp). MULTI: n sweeps behind grid barriers, one workgroup per sweep group, pagerank
// credited as the launch decides per sweep (CM = 2); otherwise ONE sweep whose crediting is a compile-time constant (CM = `owed`),
// the sweep groups beyond the grid dealt by the device counter q_take.
struct GSweepLaunch {
    int grid;                     // workgroups
    const int *cnt_in;            // frontier sizes of the live snapshot
    int *cnt_out, *cnt_zero;      // ... of the one the (last) sweep leaves; a row the launch zeroes for the one after
    int *log;                     // a row of frontier sizes per sweep
    int n;                        // sweeps
    GridBar *bar = nullptr;       // multi-sweep launches: barrier, status word, roll-call limits
    int *status = nullptr;
    unsigned long long ticks = 0;
    int rollcall_extra = 0;
    int *q_take = nullptr, *q_zero = nullptr; // one-sweep launches: the group counter to take tickets from, the one to zero
};
template <bool MULTI>
void launch_gsweep(dppr_engine *e, Group &g, const Epoch &ep, int phase, double eps, bool owed, const GSweepLaunch &a) {
    with_row(g.gw, ep.ggrp_max_tiles * WAVE, [&](auto spl, auto gw, auto nvx) {
        auto go = [&](auto cm) {
            hipLaunchKernelGGL((k_gsweep<decltype(spl)::value, decltype(gw)::value, decltype(nvx)::value, MULTI, decltype(cm)::value>),
                               dim3(a.grid), dim3(GNT), 0, e->stream, ep.grp_n_int, ep.gtab, ep.n_ggroups, a.cnt_in, e->gsweep_hot_rows,
                               ep.out_col, g.x, g.x2, g.act[0], g.act[1], g.r, g.p, a.cnt_out, a.cnt_zero, phase, eps, g.dstats + 1, a.log,
                               a.n, a.bar, a.status, a.ticks, a.rollcall_extra, owed ? 1 : 0, a.q_take, a.q_zero);
        };
        if constexpr (MULTI) go(IC<2>{});
        else if (owed) go(IC<1>{});
        else go(IC<0>{});
    });
}

// workgroups of the multi-sweep form of k_gsweep that the device holds at once
int group_multi_capacity(dppr_engine *e, int spl) {
    int &cap = e->gmulti_cap[spl - 1];
    if (cap < 0) {
        int per_cu = 0, cus = 0; // (the widest row of each lane split: narrower ones need no more)
        hipError_t rc = spl == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_gsweep<1, 8, 1024, true, 2>, GNT, 0)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_gsweep<2, 16, 512, true, 2>, GNT, 0);
        if (rc != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess)
            per_cu = 0;
        cap = std::min(per_cu * cus, STAT_SLOTS);
    }
    return cap;
}

// What group_push_tail reports: whether it took the frontier and how it ended, the iterations it ran (already in the group's
// statistics), and -- in and out -- whether the snapshot at hand still owes its pagerank share
struct PushTail {
    enum How { NOT_ENTERED, CONVERGED, GAVE_BACK } how = NOT_ENTERED;
    int iters = 0;
    bool owed = false;
};

// The tail of a group's loop in push form (dppr_gpush.hpp). Called between two chunks of sweeps when the frontier is
// small: g.act[0] / g.x hold the frontier the last sweep left. Returns CONVERGED (the loop is over; state as
// a finished loop leaves it) or GAVE_BACK (the mode gave up -- an iteration too large for it -- and put the frontier back
// in sweep form: g.act[0], g.x, frontier sizes in row 0 of g.cnt, the other rows zero), or NOT_ENTERED if it
// did not start (nothing changed). Iterations run are counted in t->iters and in the group's statistics.
// t->owed: the handed-over snapshot's pagerank share is still to be credited (the last sweep was a deferring one,
// dppr_multi.hpp); on a return in sweep form it says the same about the snapshot handed back.
int group_push_tail(dppr_engine *e, Group &g, const Epoch &ep, int phase, double eps, long long pairs_at_entry, PushTail *t) {
    const int cap = std::max(1024, std::min(e->gpush_list_cap, e->V));
    if (g.plist[0].capacity() != (size_t)cap || !g.pctl) { // (pctl comes last: a set that failed half way is made again)
        HIP_TRY(loop_wait(e));
        g.plist[0].reset(); g.plist[1].reset(); g.ppre.reset(); g.pctl.reset();
        HIP_TRY(g.plist[0].alloc((size_t)cap));
        HIP_TRY(g.plist[1].alloc((size_t)cap));
        HIP_TRY(g.ppre.alloc((size_t)cap + 1));
        HIP_TRY(g.pctl.alloc(1));
    }
    // no host round trip on the way in: a list that does not fit (overflow) moves nothing and makes the first scan call
    // the mode off, which the read-back of the first chunk shows
    HIP_TRY(hipMemsetAsync(g.pctl, 0, sizeof(GPushCtl), e->stream));
    const int n_words = (ep.grp_n_int + 31) / 32;
    hipLaunchKernelGGL(k_gpush_list, dim3(grid_for(n_words)), dim3(BLOCK), 0, e->stream, g.act[0], n_words, g.plist[0], cap, g.pctl);
    // the frontier's rows move from the snapshot back to residual[]; its bits stay set (they queue it for iteration 0)
    const int rows_grid = grid_for(std::min<long long>(pairs_at_entry, cap), BLOCK / OCT);
    with_row(g.gw, [&](auto spl, auto gw) {
        hipLaunchKernelGGL((k_gpush_rows<decltype(spl)::value, decltype(gw)::value>), dim3(rows_grid), dim3(BLOCK), 0, e->stream, g.plist[0],
                           g.pctl, 0, g.x, g.r, false);
    });
    HIP_TRY(hipGetLastError());
    static thread_local GPushCtl h;
    const int credit_first = t->owed ? 1 : 0; // (iteration 0 of this mode settles it; every later one credits as it snapshots)
    const long long max_edges = gpush_edge_bound(e->gpush_max_edges, ep.n_ggroups);
    const int grid = 256;
    static const bool trace = getenv("DPPR_GROUP_TRACE") != nullptr;
    int it_done = 0;
    long long known_n = pairs_at_entry; // (an upper bound of the frontier's vertices until the first read-back)
    bool tiny_declined = false;
    long long last_adds = gpush_adds_at_entry(pairs_at_entry); // edge x source adds of the last iteration run (-1: not known yet)
    for (;;) {
        if (gpush_take_tiny(known_n, last_adds, tiny_declined)) {
            // a frontier of a few hundred vertices: a run of iterations as ONE single-workgroup launch
            with_row(g.gw, [&](auto spl, auto gw) {
                hipLaunchKernelGGL((k_gpush_tiny<decltype(spl)::value, decltype(gw)::value>), dim3(1), dim3(1024), 0, e->stream, g.pctl, g.plist[0],
                                   g.plist[1], ep.row_ptr, ep.adj, ep.hub_degp1, g.r, g.p, g.act[0], phase, eps, g.dstats, GPUSH_LOG, credit_first);
            });
        } else {
        const int m = gpush_chunk(it_done, pairs_at_entry); // iterations of this chunk (<= GPUSH_LOG)
        tiny_declined = false;
        for (int k = 0; k < m; ++k) {
            hipLaunchKernelGGL(k_gpush_scan, dim3(1), dim3(1024), 0, e->stream, g.pctl, g.plist[0], g.plist[1], ep.row_ptr, g.ppre, cap - 1, max_edges);
            with_row(g.gw, [&](auto spl, auto gw) {
                constexpr int SPL = decltype(spl)::value, GW = decltype(gw)::value;
                hipLaunchKernelGGL((k_gpush_snap<SPL, GW>), dim3(grid), dim3(BLOCK), 0, e->stream, g.plist[0], g.plist[1], g.pctl, g.x, g.r, g.p,
                                   g.act[0], phase, eps, credit_first);
                hipLaunchKernelGGL((k_gpush_expand<SPL, GW>), dim3(grid), dim3(BLOCK), 0, e->stream, g.plist[0], g.plist[1], g.pctl, g.ppre,
                                   ep.row_ptr, ep.adj, ep.hub_degp1, g.x, g.r, g.act[0], g.plist[0], g.plist[1], cap, phase, eps, g.dstats);
            });
        }
        }
        HIP_TRY(hipGetLastError());
        // (not read_back: the chunk's control block and log come back into this function's own GPushCtl, not into e->pinned)
        HIP_TRY(hipMemcpyAsync(&h, g.pctl, sizeof(GPushCtl), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(loop_wait(e));
        for (int i = it_done; i < h.it; ++i) {
            const long long F = lane_sum(h.F[i & (GPUSH_LOG - 1)]);
            if (F == 0) continue;
            account_iteration(g.st, F, ITER_PUSH);
            ++t->iters;
            if (trace)
                fprintf(stderr, "[gpush ] phase %d iteration +%d  frontier pairs %9lld  adds %lld\n", phase, i, F, h.atomics[i & (GPUSH_LOG - 1)]);
        }
        if (gpush_tiny_declined(h.it > it_done, h.stop != 0, known_n)) tiny_declined = true; // (too many vertices or in-edges for one workgroup)
        if (h.it > it_done) last_adds = h.atomics[(h.it - 1) & (GPUSH_LOG - 1)];
        it_done = h.it;
        known_n = h.n[h.it & 1];
        if (h.stop && h.it == 0 && h.overflow) return DPPR_OK; // the frontier did not fit the lists: nothing was moved, the sweeps go on (NOT_ENTERED)
        if (h.stop) { // an iteration too large for this form: the queued vertices go back to sweep form
            if (trace) fprintf(stderr, "[gpush ] phase %d: an iteration of %d vertices called itself off after %d iterations\n", phase, h.n[h.it & 1], h.it);
            HIP_TRY(hipMemsetAsync(g.cnt, 0, sizeof(int) * 3 * GS_MAX, e->stream));
            with_row(g.gw, [&](auto spl, auto gw) {
                hipLaunchKernelGGL((k_gpush_leave<decltype(spl)::value, decltype(gw)::value>), dim3(grid_for(ep.grp_n_int, BLOCK / OCT)), dim3(BLOCK), 0,
                                   e->stream, ep.grp_n_int, g.act[0], g.x, g.r, g.p, h.it > 0 ? 1 : 0, phase, eps, g.cnt);
            });
            HIP_TRY(hipGetLastError());
            if (h.it > 0) t->owed = false; // (iteration 0 settled the hand-over, k_gpush_leave credited what it queued)
            t->how = PushTail::GAVE_BACK;
            return DPPR_OK;
        }
        if (h.n[h.it & 1] == 0) {
            t->how = PushTail::CONVERGED;
            return DPPR_OK;
        }
        if (it_done >= e->max_iters) return fail(e, DPPR_ERR_NOT_CONVERGED, "iteration cap hit");
    }
}

// One frontier loop of a source group: what its chunks share and hand to each other. Each chunk below says what it requires
// and what it leaves.
struct GroupLoop {
    dppr_engine *const e;
    Group &g;
    const Epoch &ep;
    const int phase;
    const double eps;
    const int hp = phase == PHASE_BOTH ? 0 : phase; // (loop histories: the merged loop uses slot 0)
    CounterRing ring;  // row of g.cnt that holds the live frontier sizes, one per source
    // pagerank is credited every other sweep (dppr_multi.hpp): the seeding credited its snapshot, so the first sweep defers;
    // `owed` = the live snapshot's share has not been added yet, the next sweep is a crediting one
    bool owed = false;
    int it = 0, active_iters = 0; // loop position; the position after the last iteration that saw a frontier
    bool more = false; // a frontier is left
    long long F = 0;   // ... of this many pairs, as the last chunk of one-sweep launches read them back
    // the tail of the loop as pushes (dppr_gpush.hpp): below plan.push_thr frontier pairs, one-sweep launches only
    GroupLoopPlan plan;
    int sweep_grid = 1; // workgroups of a one-sweep launch
    int *row(int k) const { return g.cnt + k * GS_MAX; }

    // requires a window whose sweep groups are all resident at once; leaves a run of sweeps done as ONE launch (k_gsweep<.., true>)
    // and accounted, and if it ran out of sweeps the live sizes in row 0 -- or, after a failed roll-call, nothing changed and
    // one-sweep launches from here on (re-armed later)
    int multi_chunk() {
        const int n = group_multi_sweeps(g.hist.hint[hp], it, e->chunk_iters, e->chunk_explicit);
        HIP_TRY(hipMemsetAsync(g.mlog, 0, sizeof(int) * (size_t)(n + 2) * GS_MAX, e->stream));
        HIP_TRY(hipMemsetAsync(e->bar, 0, sizeof(GridBar), e->stream));
        int rc = timed_launch(e, 0, e->profiling, [&] { // (g.mlog: the status word's row, then a row of frontier sizes per sweep)
            launch_gsweep<true>(e, g, ep, phase, eps, owed,
                                {ep.n_ggroups, row(ring.cur), row(3), row(4), g.mlog + GS_MAX, n, e->bar, g.mlog, e->persist_ticks, e->persist_rollcall_extra});
        });
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        if ((rc = read_back(e, g.mlog, (size_t)(n + 2) * GS_MAX))) return rc;
        const int st = e->pinned[0];
        g.st.persist_launches++;
        if (st & GSM_FAULT) return fail(e, DPPR_ERR_HIP, "a grid barrier of the multi-sweep group launch timed out");
        if (st & GSM_ABORTED) {
            give_up_resident(e, g.st);
            return DPPR_OK;
        }
        const int sweeps = st & GSM_SWEEPS;
        account_sweeps(g.st, e->pinned + GS_MAX, sweeps, GS_MAX, ITER_SWEEP, it, &active_iters); // (the launch ran no sweep on an empty frontier)
        if (e->profiling && (rc = credit_launch(e, g.st, 0, false))) return rc;
        if (sweeps & 1) { // (no rotation: the launch keeps its own counters, rows 3 and 4)
            swap_snapshots(g, true);
            owed = !owed;
        }
        it += sweeps;
        more = !(st & GSM_CONVERGED);
        if (!more) return DPPR_OK;
        // out of sweeps: the live frontier sizes are in row `sweeps`; the launch left them in cnt[3] -- make them cnt[0]
        HIP_TRY(hipMemcpyAsync(row(0), row(3), sizeof(int) * GS_MAX, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemsetAsync(row(1), 0, sizeof(int) * 2 * GS_MAX, e->stream));
        ring.cur = 0;
        more = lane_sum(e->pinned + GS_MAX + sweeps * GS_MAX) > 0;
        return DPPR_OK;
    }
    // requires e->pinned to hold the live frontier sizes in row ring.cur; leaves a chunk of one-sweep launches
    // (GroupLoopPlan::next_chunk) enqueued, read back and accounted, all of g.cnt in e->pinned, and F / more on what they left
    int sweep_chunk() {
        const int n = plan.next_chunk(g.hist, hp, it, lane_sum(e->pinned + ring.cur * GS_MAX), e->chunk_iters, e->chunk_explicit);
        for (int k = 0; k < n; ++k) {
            int rc = timed_launch(e, k, e->profiling, [&] {
                launch_gsweep<false>(e, g, ep, phase, eps, owed,
                                     {sweep_grid, row(ring.cur), row(ring.nxt()), row(ring.zer()), row(5 + k), 1, nullptr, nullptr, 0, 0,
                                      g.gq + (g.gq_seq % 3) * GQ_PAD, g.gq + ((g.gq_seq + 1) % 3) * GQ_PAD});
            });
            if (rc) return rc;
            swap_snapshots(g, true);
            ring.rotate();
            g.gq_seq++;
            owed = !owed; // (if the frontier emptied on the way, the later launches do nothing and nothing is owed: `more` is false below)
        }
        HIP_TRY(hipGetLastError());
        if (int rc = read_back(e, g.cnt, (size_t)(5 + n) * GS_MAX)) return rc; // (the per-chunk log follows the five counter rows)
        int rc = account_sweeps(g.st, e->pinned + 5 * GS_MAX, n, GS_MAX, ITER_SWEEP, it, &active_iters, [&](int k, long long f) -> int {
            plan.saw_frontier(f, it + k);
            if (!e->profiling) return DPPR_OK;
            float ms = 0;
            if (int rc2 = credit_launch(e, g.st, k, true, &ms)) return rc2;
            static const bool trace = getenv("DPPR_GROUP_TRACE") != nullptr; // (diagnostic: one line per sweep)
            if (trace) fprintf(stderr, "[gsweep] phase %d sweep %3d  frontier pairs %9lld  %7.1f us\n", phase, it + k, f, ms * 1e3);
            return DPPR_OK;
        });
        if (rc) return rc;
        F = lane_sum(e->pinned + ring.cur * GS_MAX);
        more = F > 0;
        it += n;
        return DPPR_OK;
    }
    // requires a chunk just read back with F pairs left, few enough for the push form (GroupLoopPlan::enter_push); leaves the
    // tail of the loop run as pushes (group_push_tail) -- or, where that form gave the frontier back or did not take it, the
    // frontier in sweep form with its sizes read back, and a much lower threshold for the next try
    int hand_to_push_tail() {
        plan.saw_frontier(F, it);
        PushTail t;
        t.owed = owed;
        if (int rc = group_push_tail(e, g, ep, phase, eps, F, &t)) return rc;
        owed = t.owed;
        if (t.how != PushTail::NOT_ENTERED) {
            active_iters = it + t.iters;
            it += t.iters;
        }
        if (t.how == PushTail::CONVERGED) more = false;
        else plan.push_declined(F);
        if (t.how != PushTail::GAVE_BACK) return DPPR_OK;
        ring.cur = 0; // back in sweep form: frontier sizes in row 0
        if (int rc = read_back(e, row(0), GS_MAX)) return rc;
        more = lane_sum(e->pinned) > 0;
        return DPPR_OK;
    }
};

// One frontier loop of a source group. `tails`: the state was converged before the batch's stream
// update, so only the batch tails (grouped in batch_tails: each tail one run, dppr_grouping.hpp) can be legal -- no pass over all vertices.
int group_loop(dppr_engine *e, Group &g, const Epoch &ep, int phase, double eps, bool tails) {
    GroupLoop l{e, g, ep, phase, eps};
    HIP_TRY(hipMemsetAsync(g.cnt, 0, sizeof(int) * 3 * GS_MAX, e->stream));
    if (tails) {
        HIP_TRY(hipMemsetAsync(g.act[0], 0, g.act_bytes, e->stream));
        if (ep.L > 0) {
            with_row(g.gw, [&](auto spl, auto gw) {
                hipLaunchKernelGGL((k_gseed_tails<decltype(spl)::value, decltype(gw)::value>), dim3(grid_for(ep.L, BLOCK / OCT)), dim3(BLOCK), 0,
                                   e->stream, batch_tails(e, ep), ep.L, g.r, g.x, g.p, g.act[0], phase, eps, l.row(0));
            });
        }
    } else {
        // dense seeding: every legal vertex of every source enters, snapshot taken
        with_row(g.gw, [&](auto spl, auto gw) {
            hipLaunchKernelGGL((k_gseed_dense<decltype(spl)::value, decltype(gw)::value>), dim3(grid_for(ep.grp_n_int, BLOCK / OCT)), dim3(BLOCK), 0,
                               e->stream, ep.grp_n_int, g.r, g.x, g.p, g.act[0], phase, eps, l.row(0));
        });
        g.st.inspected += (int64_t)ep.grp_n_int * g.n;
    }
    HIP_TRY(hipGetLastError());
    int rc = read_back(e, l.row(0), GS_MAX);
    if (rc) return rc;
    l.more = lane_sum(e->pinned) > 0;
    if (e->gsweep_grid_cap <= 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus <= 0) cus = 256;
        e->gsweep_grid_cap = std::min(2 * cus, STAT_SLOTS);
    }
    l.sweep_grid = std::min(std::max(ep.n_ggroups, 1), e->gsweep_grid_cap);
    l.plan.push_thr = group_push_threshold(e->gpush_enter_pairs, ep.n_ggroups, e->gpush_auto_factor);
    while (l.more) {
        if (l.it >= e->max_iters) return fail(e, DPPR_ERR_NOT_CONVERGED, "iteration cap hit");
        // a window whose sweep groups are all resident at once: a run of sweeps as ONE launch; otherwise one-sweep launches in chunks
        const int mcap = e->group_resident && e->persist_mode && e->persist_ok && e->chunk_iters > 1 ? group_multi_capacity(e, g.spl) : 0;
        if (mcap > 0 && ep.n_ggroups > 0 && ep.n_ggroups <= mcap) rc = l.multi_chunk();
        else if (!(rc = l.sweep_chunk()) && l.plan.enter_push(l.more, l.F)) rc = l.hand_to_push_tail();
        if (rc) return rc;
    }
    l.plan.finish(g.hist, l.hp, l.active_iters);
    return DPPR_OK;
}

// One freshly initialised column of an otherwise converged group (dppr_churn.hpp: p = 0, r = e_src in that lane), solved on
// `ep`: Init + ExecuteMainLoop(0) for that source, as dppr_group_init_solve_at runs them for all. The tolerance is the group's
// own, so dense seeding finds exactly the one legal vertex -- every other column satisfies |r| <= conv_eps and stays inert in
// every sweep (the legal-push test is per source). The loop histories size the first chunk of the NEXT UPDATE's loops, and a
// from-scratch loop is no predictor of those: they are put back.
int group_solve_column(dppr_engine *e, Group &g, const Epoch &ep) {
    const LoopHistory kept = g.hist;
    const int rc = group_loop(e, g, ep, 0, g.conv_eps, /*tails=*/false);
    g.hist = kept;
    return rc;
}

int group_stream_update(dppr_engine *e, Group &g, const Epoch &ep) {
    const int L = ep.L;
    if (L == 0) return DPPR_OK;
    int rc = group_records_by_tail(e, ep, nullptr, 0, nullptr, 0);
    if (rc) return rc;
    SuSources srcs{};
    for (int s = 0; s < GS_MAX; ++s) srcs.s[s] = g.src.s[s];
    // blockIdx.y = source lane; state element (v, lane) at base[v * gw + lane]
    hipLaunchKernelGGL(k_su_terms, dim3(grid_for(L), g.n), dim3(BLOCK), 0, e->stream, batch_tails(e, ep), batch_order(e, ep), ep.b2,
                       ep.ins, L, g.p, g.gw, e->su_term, e->su_ins);
    if (g.tsets.n > 0) // a group with a set lane: the source term of a tail is ALPHA * h[u] from the seed table (dppr_targets.hpp)
        hipLaunchKernelGGL(k_su_apply_seeded, dim3(grid_for(L), g.n), dim3(BLOCK), 0, e->stream, batch_tails(e, ep), batch_order(e, ep),
                           e->su_term, e->su_ins, ep.deg_after, L, g.r, g.gw, tg_dev(g));
    else
        hipLaunchKernelGGL(k_su_apply, dim3(grid_for(L), g.n), dim3(BLOCK), 0, e->stream, batch_tails(e, ep), batch_order(e, ep), e->su_term,
                           e->su_ins, ep.deg_after, L, g.r, g.gw, srcs, 0.0, (int *)nullptr, (int *)nullptr, (int *)nullptr,
                           (int *)nullptr);
    HIP_TRY(hipGetLastError());
    g.st.records += (int64_t)L * g.n;
    return DPPR_OK;
}

// One batch of a source group = dppr_group_update: the stream update of every source and the loops, inside the event bracket
int group_update(dppr_engine *e, Group &g, Epoch &ep, double eps, float *out_ms) {
    // seeding from the batch tails is exact only if every |r| <= eps beforehand (slot_update has the same rule)
    const bool merged = e->merge_phases && e->schedule == DPPR_SCHEDULE_EAGER; // (dppr_set_phase_merge)
    if (merged) eps = eps / e->merge_div;
    const bool tails = g.converged && g.conv_eps <= eps && e->group_tail_seeding;
    int rc = settle_parked(e, g.p, g.r, g.gw, eps, &g.park_eps, &g.st);
    if (rc) return rc;
    rc = prepare_epoch(e, ep);
    if (rc) return rc;
    rc = bracket_open(e);
    if (rc) return rc;
    rc = group_stream_update(e, g, ep);
    if (rc) return rc;
    g.converged = false;
    if (merged) rc = group_loop(e, g, ep, PHASE_BOTH, eps, tails);
    else if (!(rc = group_loop(e, g, ep, 0, eps, tails))) rc = group_loop(e, g, ep, 1, eps, tails);
    if (rc) return rc;
    return solve_finished(e, g, eps, ep.id, true, out_ms);
}

} // namespace
