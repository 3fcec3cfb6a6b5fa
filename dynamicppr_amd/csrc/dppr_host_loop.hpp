// dppr_host_loop.hpp -- host side, part 3 of 4: the single-source SOLVER. IncrementalBatchUpdate's grouping and replay
// (gpu/StreamUpdate.cuh:7-76), the frontier loop of PPRRevPushGPU::ExecuteOptimized (gpu/PPRRevPushGPU.cuh:97-131) with its launch
// forms -- push iterations, per-iteration sweeps (gather or binned), resident launches of a run of sweeps or of a whole batch --
// and the sequence of one batch (slot_update). What to launch and what follows a launch is decided in dppr_loop_plan.hpp; the
// functions here enqueue, read back and account. Runs on the engine's solver stream.
#pragma once

namespace {

template <int N> using IC = std::integral_constant<int, N>; // (a block size, row width, ... handed to a launch as a compile-time constant)

// ---- the steps every loop shares, single source and source group alike
// n ints from device memory are in e->pinned when this returns (a read-back of a loop: a sign of life, loop_wait)
int read_back(dppr_engine *e, const void *dptr, size_t n) {
    HIP_TRY(hipMemcpyAsync(e->pinned, dptr, sizeof(int) * n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(loop_wait(e));
    return DPPR_OK;
}
int read_count(dppr_engine *e, const int *dptr, int *out) {
    if (int rc = read_back(e, dptr, 1)) return rc;
    *out = e->pinned[0];
    return DPPR_OK;
}
inline long long pinned_u64(const dppr_engine *e, int word) { // (a 64-bit counter that came back at that int of e->pinned)
    unsigned long long d;
    memcpy(&d, e->pinned + word, sizeof(d));
    return (long long)d;
}

// launch k of a chunk between the events of its pair (`timed`: profiling, or the push / sweep pricing wants its time) ...
template <class Launch>
int timed_launch(dppr_engine *e, int k, bool timed, Launch &&launch) {
    if (timed) HIP_TRY(hipEventRecord(e->evpool[2 * k], e->stream));
    launch();
    if (timed) HIP_TRY(hipEventRecord(e->evpool[2 * k + 1], e->stream));
    return DPPR_OK;
}
// ... and what it took, once the chunk was read back, in the profile: every launch of a loop counts as a push launch, ONE sweep
// also as a sweep launch (the sweep kernel's roofline; resident and multi-sweep launches are none)
inline int credit_launch(dppr_engine *e, dppr_stats_t &st, int k, bool one_sweep, float *ms_out = nullptr) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->evpool[2 * k], e->evpool[2 * k + 1]));
    st.push_ms += ms;
    st.push_launches++;
    if (one_sweep) {
        st.sweep_ms += ms;
        st.sweep_launches++;
    }
    if (ms_out) *ms_out = ms;
    return DPPR_OK;
}

// a roll-call failed (the grid was not co-resident): the launch changed nothing; this engine goes on with one launch per
// iteration (a later slot_update re-arms the resident forms after PERSIST_RETRY_BATCHES; group_update never does)
inline void give_up_resident(dppr_engine *e, dppr_stats_t &st) {
    st.persist_aborts++;
    e->persist_ok = false;
    e->persist_retry = PERSIST_RETRY_BATCHES;
}

// The three rotating counters of a loop: a launch takes the live frontier size from `cur`, counts the next frontier into nxt()
// and zeroes zer() for the launch after it
struct CounterRing {
    int cur = 0;
    int nxt() const { return (cur + 1) % 3; }
    int zer() const { return (cur + 2) % 3; }
    void rotate() { cur = nxt(); }
};
// a sweep wrote every entry of x2 (`bits`: and the activity bitmap act[1]): they are the next snapshot
template <class State>
void swap_snapshots(State &o, bool bits) {
    std::swap(o.x, o.x2);
    if (bits) std::swap(o.act[0], o.act[1]);
}

// ---- accounting of a read-back log: `width` frontier sizes per logged iteration (a source group: one per source)
inline long long lane_sum(const int *row, int width = GS_MAX) {
    long long F = 0;
    for (int s = 0; s < width; ++s) F += row[s];
    return F;
}

enum IterKind { ITER_PUSH, ITER_RESIDENT_SWEEP, ITER_SWEEP }; // (a resident launch's edges are counted with the pushes': no sweep_F)

inline void account_iteration(dppr_stats_t &st, long long F, IterKind kind) {
    st.iterations++;
    st.sum_F += F;
    if (kind != ITER_PUSH) st.pull_iterations++;
    if (kind == ITER_SWEEP) st.sweep_F += F;
}

// Every one of the n logged iterations that saw a frontier counts: iterations, sum_F, by kind pull_iterations and sweep_F;
// *active_iters becomes the loop position after the last of them (the log starts at position `it`). each(k, F) is called for
// every such iteration (per-launch timings, traces); a status other than DPPR_OK ends the walk and is returned.
template <class Each>
int account_sweeps(dppr_stats_t &st, const int *rows, int n, int width, IterKind kind, int it, int *active_iters, Each &&each) {
    for (int k = 0; k < n; ++k) {
        const long long F = lane_sum(rows + (size_t)k * width, width);
        if (F <= 0) continue; // the frontier emptied inside the chunk: the rest were no-ops
        account_iteration(st, F, kind);
        *active_iters = it + k + 1;
        if (int rc = each(k, F)) return rc;
    }
    return DPPR_OK;
}
inline void account_sweeps(dppr_stats_t &st, const int *rows, int n, int width, IterKind kind, int it, int *active_iters) {
    account_sweeps(st, rows, n, width, kind, it, active_iters, [](int, long long) -> int { return DPPR_OK; });
}

int pull_min_frontier(const dppr_engine *e) { return dppr::pull_min_frontier(e->pull_min_frontier, e->Ed); }

// The sweep kernels are instantiated per workgroup size (= max tiles per sweep group x 64: the groups themselves were cut by
// the builder): f(PB) is called with it as a compile-time constant. ANY: every size dppr_set_tuning takes -- the bitmap form
// of k_pull_iter alone; a size that is not 256 / 512 / 1024 never runs resident and always takes that form.
template <bool ANY, class F>
void with_block(int pb, F &&f) {
    switch (pb) {
    case 256: return f(IC<256>{});
    case 512: return f(IC<512>{});
    case 1024: return f(IC<1024>{});
    }
    if constexpr (ANY) {
        switch (pb) {
        case 384: return f(IC<384>{});
        case 576: return f(IC<576>{});
        case 640: return f(IC<640>{});
        case 768: return f(IC<768>{});
        case 896: return f(IC<896>{});
        }
    }
    f(IC<1024>{});
}

// k_pull_resident (dppr_resident.hpp) at the sweep's block size: n sweeps from counter `cur` on; plan: PLAN_* of a whole-batch
// launch (0: a run of sweeps of one loop), upd: the batch's records if the launch applies them itself
void launch_resident(dppr_engine *e, Slot &s, const Epoch &ep, double eps, int cur, int phase, int n, int plan, const ResUpdate &upd) {
    with_block<false>(sweep_block(e), [&](auto pb) {
        hipLaunchKernelGGL(k_pull_resident<decltype(pb)::value>, dim3(ep.n_groups), dim3(decltype(pb)::value), 0, e->stream, ep.grp_n_int,
                           ep.grp_tile, ep.out_row_ptr, ep.out_col, s.x, e->res_arena, e->res_arena_stride, s.r, s.p, s.cnt, cur, phase, eps,
                           s.dstats, s.log, n, e->bar, s.cnt + 7, e->persist_ticks, e->persist_rollcall_extra, plan,
                           ep.res_valid ? ep.res_pk : nullptr, upd);
    });
}
// ... timed where profiling is on; the counters, the status word (s.cnt[7]) and the log of n entries are in e->pinned afterwards
int run_resident(dppr_engine *e, Slot &s, const Epoch &ep, double eps, int cur, int phase, int n, int plan, const ResUpdate &upd) {
    if (int rc = timed_launch(e, 0, e->profiling, [&] { launch_resident(e, s, ep, eps, cur, phase, n, plan, upd); })) return rc;
    HIP_TRY(hipGetLastError());
    return read_back(e, s.cnt, (size_t)(CNT_HDR + n));
}

// One frontier loop of a single source (run_frontier_loop, below): what its steps share and hand to each other. Each step says what
// it requires and what it leaves.
struct FrontierLoop {
    dppr_engine *const e;
    Slot &s;
    const Epoch &ep;
    const int phase;
    const double eps;
    int buf;           // s.ft[buf]: the frontier's list (where form.list)
    CounterRing ring;  // s.cnt[ring.cur]: its size
    FrontierForm form; // which of list and snapshot is live
    int F, prevF = 0;  // the frontier's size as last read back, and the one read before it
    long long D = -1;  // in-edges of the frontier (binned windows), -1 = not counted
    int follow = 4;    // size of the next follow-up chunk of per-iteration sweeps
    int it, active_iters; // loop position; the position after the last iteration that saw a frontier
    // fixed when the loop starts (set in the constructor, in this order: each may read the ones before it)
    int pull_min, pcap0, push_grid;
    bool sync_sched, binned, use_bits, use_status;
    const HubTable hubs{ep.hub_v, ep.hub_degp1, ep.n_hubs};
    unsigned long long *const dsum = reinterpret_cast<unsigned long long *>(s.cnt + 8); // three slots beside the rotating counters

    FrontierLoop(dppr_engine *e_, Slot &s_, const Epoch &ep_, int phase_, double eps_, int buf_, int cur_, const LoopEntry &en)
        : e(e_), s(s_), ep(ep_), phase(phase_), eps(eps_), buf(buf_), ring{cur_}, form(en), F(en.F), it(en.it), active_iters(en.it) {
        pull_min = pull_min_frontier(e);
        pcap0 = persist_capacity(e);
        sync_sched = e->schedule == DPPR_SCHEDULE_SYNC;
        // the sparse grid must cover the largest frontier a push chunk can meet
        push_grid = pull_min == PULL_NEVER ? 2048 : std::min(2048, std::max(64, (pull_min * 4 / WAVE + 3) / 4));
        binned = ep.bin_valid && ep.bin_n_int <= ep.grp_n_int && (pcap0 <= 0 || ep.n_groups > pcap0 || e->bin_mode == 2);
        // Sweeps on a window that cannot run resident carry the activity bitmap of their snapshot (k_pull_iter<.., true>)
        use_bits = e->sweep_bits && !binned && !en.dense && (pcap0 <= 0 || ep.n_groups > pcap0);
        // The merged loop always filters through the status array: adds of both signs can take a residual across the threshold more
        // than once per iteration, and with the crossing test every crossing would append -- the next-frontier list (V entries) could
        // overflow. One entry per vertex and launch keeps it bounded.
        use_status = e->status_dedup || phase == PHASE_BOTH;
    }

    // requires the list in s.ft[buf] or the snapshot in s.x (after a sweep); leaves the list, made from the snapshot if need be
    int need_list() {
        if (!form.needs_list()) return DPPR_OK;
        HIP_TRY(hipMemsetAsync(s.cnt + 7, 0, sizeof(int), e->stream));
        hipLaunchKernelGGL(k_list_from_dense, dim3(grid_for(ep.grp_n_int, BLOCK * INSPECT_ITEMS)), dim3(BLOCK), 0, e->stream,
                           s.x, ep.grp_n_int, s.cnt + ring.cur, s.ft[buf], s.cnt + 7);
        HIP_TRY(hipGetLastError());
        form.list_made();
        return DPPR_OK;
    }
    // requires the list in s.ft[buf]; leaves its snapshot in s.x (bm: and its activity bitmap in s.act[0]; extr: the residuals it took
    // zeroed). Grid-stride over a frontier whose size is only known on the device (k > 0): sized for the last size the host saw, capped
    int take_snapshot(bool bm, bool extr) {
        if (bm) HIP_TRY(hipMemsetAsync(s.act[0], 0, s.act_bytes, e->stream));
        hipLaunchKernelGGL(k_snapshot_dense, dim3(std::min(grid_for(std::max(F, 1 << 14)), 1024)), dim3(BLOCK), 0, e->stream, s.ft[buf],
                           s.cnt + ring.cur, s.r, s.p, s.x, bm ? s.act[0] : (uint32_t *)nullptr, phase == PHASE_BOTH ? 1 : 0, extr ? 1 : 0);
        form.snapshot_taken(extr);
        return DPPR_OK;
    }
    // requires F > 0 as read back; leaves the frontier's external ids appended to the slot's trace (a blocking copy of the list)
    int trace_frontier() {
        if (int rc = need_list()) return rc;
        size_t old = s.trace_ids.size();
        s.trace_ids.resize(old + (size_t)F);
        // (not read_back: the ids go to the trace's own memory, not to e->pinned)
        HIP_TRY(hipMemcpyAsync(s.trace_ids.data() + old, s.ft[buf], sizeof(int) * (size_t)F, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(loop_wait(e));
        for (size_t i = old; i < s.trace_ids.size(); ++i) s.trace_ids[i] = e->int2ext[(size_t)s.trace_ids[i]];
        s.trace_off.push_back((int64_t)s.trace_ids.size());
        return DPPR_OK;
    }
    // requires *pull = the decision by vertex count; leaves it replaced by what each form would cost where the window is priced (dppr_loop_plan.hpp).
    // The frontier's in-edges D are counted by the sweep that left it (k_bin_reduce) or, for a list, here by k_front_degree (one more read-back)
    int price(bool costly, bool *pull) {
        if (!costly || !e->cost_model || sync_sched || s.trace || e->pull_min_frontier != 0) return DPPR_OK;
        if (cost_needs_degrees(F, D)) {
            if (int rc = need_list()) return rc;
            HIP_TRY(hipMemsetAsync(dsum + ring.cur, 0, sizeof(unsigned long long), e->stream));
            hipLaunchKernelGGL(k_front_degree, dim3(grid_for(F)), dim3(BLOCK), 0, e->stream, s.ft[buf], s.cnt + ring.cur, ep.row_ptr, dsum + ring.cur);
            HIP_TRY(hipGetLastError());
            if (int rc = read_back(e, dsum + ring.cur, 2)) return rc;
            D = pinned_u64(e, 0);
        }
        if (cost_decides(F, D)) *pull = cost_says_sweep(F, D, s.sweep_us, ep.Ed, s.atomic_ns);
        return DPPR_OK;
    }
    // requires a chunk of n >= 2 sweeps on a window whose groups fit the chip; leaves them run as ONE resident launch (dppr_resident.hpp) and
    // accounted, the live count in cnt[0], the last sweep's snapshot in s.x -- or, after a failed roll-call, nothing changed and that form given up
    int resident_run(int n) {
        if (form.needs_snapshot())
            if (int rc = take_snapshot(false, false)) return rc;
        HIP_TRY(hipMemsetAsync(e->bar, 0, sizeof(GridBar), e->stream));
        if (int rc = run_resident(e, s, ep, eps, ring.cur, phase, n, 0, ResUpdate{})) return rc;
        const int status = e->pinned[7];
        s.st.persist_launches++;
        if (status & PERSIST_FAULT) return fail(e, DPPR_ERR_HIP, "grid barrier of the resident sweep timed out");
        if (status & PERSIST_ABORTED) {
            give_up_resident(e, s.st);
            return DPPR_OK;
        }
        account_sweeps(s.st, e->pinned + CNT_HDR, n, 1, ITER_RESIDENT_SWEEP, it, &active_iters);
        if (e->profiling)
            if (int rc = credit_launch(e, s.st, 0, false)) return rc;
        ring.cur = 0;
        form.resident_returned((status & PERSIST_CONVERGED) != 0);
        prevF = F;
        F = e->pinned[0];
        it += n;
        return DPPR_OK;
    }
    // requires the list in s.ft[buf] (synchronous schedule: and its snapshot); leaves one push iteration enqueued (k_push_iter +
    // the deferred big rows, k_push_big): the next list in s.ft[buf ^ 1], the snapshot consumed
    void push_iteration(int *log_slot) {
        int *big_cnt = s.cnt + 5 + (int)(s.iter_seq & 1), *big_zero = s.cnt + 5 + (int)((s.iter_seq + 1) & 1);
        s.iter_seq++;
        const Dedup dd{use_status ? s.status : nullptr, (int)(s.iter_seq & 0x3fffffff)};
        int *nxt = s.cnt + ring.nxt(), *zer = s.cnt + ring.zer();
        auto launch = [&](auto dense) { // (k_push_iter<false> is handed no repair flag: only a snapshot can have extracted)
            hipLaunchKernelGGL(k_push_iter<decltype(dense)::value>, dim3(push_grid), dim3(BLOCK), 0, e->stream, s.ft[buf], s.cnt + ring.cur, s.ft[buf ^ 1],
                               nxt, zer, s.x, ep.row_ptr, ep.adj, hubs, s.big, big_cnt, big_zero, e->big_row, s.r, s.p, phase, eps, s.dstats, log_slot, dd,
                               form.extracted ? 1 : 0);
        };
        if (form.dense) launch(std::true_type{});
        else launch(std::false_type{});
        hipLaunchKernelGGL(k_push_big, dim3(512), dim3(BLOCK), 0, e->stream, s.big, big_cnt, s.ft[buf ^ 1], nxt, ep.adj, hubs, s.r, phase, eps,
                           s.dstats, dd);
        form.pushed();
    }
    // requires the snapshot in s.x (use_bits: with its bitmap); leaves one gather sweep enqueued (k_pull_iter): the next snapshot
    // in s.x again, the frontier counted but not listed
    void gather_sweep(int *log_slot) {
        auto launch = [&](auto pb, auto bits) {
            hipLaunchKernelGGL((k_pull_iter<decltype(pb)::value, decltype(bits)::value>), dim3(std::min(std::max(ep.n_groups, 1), 1024)),
                               dim3(decltype(pb)::value), 0, e->stream, ep.grp_n_int, ep.grp_tile, ep.n_groups, s.cnt + ring.cur, ep.out_row_ptr,
                               ep.out_col, s.x, s.x2, s.r, s.p, s.cnt + ring.nxt(), s.cnt + ring.zer(), phase, eps, s.dstats + 1, log_slot,
                               std::min(e->big_row, PULL_BIG_ROW_DEFAULT), s.act[0], s.act[1]);
        };
        if (use_bits) with_block<true>(sweep_block(e), [&](auto pb) { launch(pb, std::true_type{}); });
        else with_block<false>(sweep_block(e), [&](auto pb) { launch(pb, std::false_type{}); });
        swap_snapshots(s, use_bits);
        form.swept();
    }
    // requires the snapshot in s.x; leaves one binned sweep enqueued, two streaming passes over the epoch's binned edge layout
    // (dppr_binned.hpp): the next snapshot in s.x again (costly: and the in-edges of the frontier it leaves in dsum[nxt])
    void binned_sweep(int *log_slot, bool costly) {
        if (ep.n_chunks > 0)
            hipLaunchKernelGGL(k_bin_scatter, dim3(ep.n_chunks), dim3(BIN_NT), (size_t)e->bin_ha_tiles * WAVE * sizeof(double), e->stream,
                               ep.bin_n_int, s.cnt + ring.cur, ep.acut, ep.chunks, ep.hl, ep.tb, ep.tdelta, ep.n_runs, s.x, e->bin_vals);
        const int rows_cap = e->bin_hb_tiles * WAVE;
        hipLaunchKernelGGL(k_bin_reduce, dim3(ep.n_b + (ep.grp_n_int - ep.bin_n_int + rows_cap - 1) / rows_cap), dim3(BIN_NT),
                           (size_t)rows_cap * 20, e->stream, ep.grp_n_int, ep.bin_n_int, ep.n_b, s.cnt + ring.cur, ep.bcut, rows_cap, ep.out_row_ptr,
                           ep.dl, ep.vb, ep.Ed, e->bin_vals, s.x, s.x2, s.r, s.p, s.cnt + ring.nxt(), s.cnt + ring.zer(), phase, eps, s.dstats + 1,
                           log_slot, e->directed ? ep.row_ptr : (const int *)nullptr, costly ? dsum + ring.nxt() : (unsigned long long *)nullptr);
        swap_snapshots(s, false);
        form.swept();
    }
    // requires a chunk of n iterations of one kind, decided; leaves them enqueued, one launch (pair) per iteration, each between
    // its events where it is timed (profiling; a priced iteration that runs alone)
    int enqueue_chunk(int n, bool pull, bool costly) {
        const bool timed = e->profiling || (costly && n == 1); // (the push / sweep decision prices both by what the last ones took)
        for (int k = 0; k < n; ++k) {
            if ((pull || sync_sched) && form.needs_snapshot()) // (a sweep repairs by itself, rn -= x[v]: it extracts nothing)
                if (int rc = take_snapshot(use_bits && pull, e->pre_extract && !pull)) return rc;
            if (costly) HIP_TRY(hipMemsetAsync(dsum + ring.nxt(), 0, sizeof(unsigned long long), e->stream));
            int rc = timed_launch(e, k, timed, [&] {
                if (pull && binned) binned_sweep(s.log + k, costly);
                else if (pull) gather_sweep(s.log + k);
                else push_iteration(s.log + k);
            });
            if (rc) return rc;
            buf ^= 1;
            ring.rotate();
        }
        HIP_TRY(hipGetLastError());
        return DPPR_OK;
    }
    // requires those n iterations enqueued; leaves them read back (ONE read-back per chunk: the counters and the F of each iteration) and
    // accounted -- statistics, profile, trace line, the pricing's running means -- and F / prevF / D / it on the frontier they left
    int finish_chunk(int n, bool pull, bool costly) {
        if (int rc = read_back(e, s.cnt, (size_t)(CNT_HDR + n))) return rc;
        int rc = account_sweeps(s.st, e->pinned + CNT_HDR, n, 1, pull ? ITER_SWEEP : ITER_PUSH, it, &active_iters, [&](int k, long long f) -> int {
            if (pull && binned) s.st.binned_sweeps++;
            if (!e->profiling) return DPPR_OK;
            float ms = 0;
            if (int rc2 = credit_launch(e, s.st, k, pull, &ms)) return rc2;
            static const bool trace = getenv("DPPR_LOOP_TRACE") != nullptr; // (diagnostic: one line per iteration of a profiled batch)
            if (trace)
                fprintf(stderr, "[loop  ] phase %d iteration %3d  %-6s frontier %9lld  %8.1f us\n", phase, it + k,
                        pull ? (binned ? "binned" : "sweep") : "push", f, ms * 1e3);
            return DPPR_OK;
        });
        if (rc) return rc;
        if (costly && n == 1 && e->pinned[CNT_HDR] > 0) { // what a sweep of this window costs / what an atomic of a push does (running means)
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, e->evpool[0], e->evpool[1])); // (the pair of launch 0, read again: this is no profile entry)
            if (pull) s.sweep_us = mean_sweep_us(s.sweep_us, ms);
            else s.atomic_ns = mean_atomic_ns(s.atomic_ns, ms, D);
        }
        prevF = F;
        F = e->pinned[ring.cur];
        D = binned && pull ? pinned_u64(e, 8 + 2 * ring.cur) : -1; // (the sweep counted the in-edges of the frontier it left)
        it += n;
        return DPPR_OK;
    }
};

// Frontier loop: PPRRevPushGPU::ExecuteOptimized's while(1) (gpu/PPRRevPushGPU.cuh:106-130).
// On entry s.ft[buf] holds the frontier and s.cnt[cur] its size; cnt[(cur+1)%3] is zero and
// the dense vectors s.x / s.x2 are all zero (no snapshot taken yet) -- unless `entry` says
// otherwise.
//
// The reference reads the frontier count back after EVERY iteration (blocking 4-byte D2H,
// :107). Here iterations are enqueued in CHUNKS: every kernel takes F from device memory,
// rotates the three counters itself and exits at once when F == 0, so the host only reads
// the count (and the per-iteration log of F) once per chunk. The host also picks, per chunk,
// how the iterations are evaluated: SPARSE (push kernels, atomics) or DENSE (pull sweep, no
// atomics; as ONE resident launch for the whole chunk when the epoch's sweep groups fit the chip,
// dppr_resident.hpp) -- the same sums either way.
//
// `entry` (LoopEntry, dppr_loop_plan.hpp) describes a loop that is picked up in the middle (after a
// launch of batch_ahead that ended before the loop did).
int run_frontier_loop(dppr_engine *e, Slot &s, const Epoch &ep, int phase, double eps, int buf, int cur,
                      LoopEntry entry = LoopEntry()) {
    const int hp = phase == PHASE_BOTH ? 0 : phase; // (loop histories: the merged loop uses slot 0)
    FrontierLoop l(e, s, ep, phase, eps, buf, cur, entry);
    if (l.use_status && !s.status) { // (first use: -1 everywhere = "never queued")
        HIP_TRY(s.status.alloc((size_t)e->V));
        HIP_TRY(hipMemsetAsync(s.status, 0xff, sizeof(int) * (size_t)e->V, e->stream));
    }
    int rc = DPPR_OK;
    if (l.F < 0 && (rc = read_count(e, s.cnt + cur, &l.F))) return rc;
    if (entry.it == 0) {
        s.start_dense[hp] = l.F >= l.pull_min;
        s.last_F0[hp] = l.F;
    }
    while (l.F > 0) {
        if (l.it >= e->max_iters) return fail(e, DPPR_ERR_NOT_CONVERGED, "iteration cap hit");
        if (s.trace && (rc = l.trace_frontier())) return rc;
        bool pull = l.F >= l.pull_min;
        // a window whose iterations cost hundreds of microseconds and more (twitter / friendster size): decisions per iteration
        const bool costly = window_costly(l.binned, e->chunk_explicit, s.sweep_us, ep.Ed);
        if ((rc = l.price(costly, &pull))) return rc;
        int n = single_chunk(s.trace, e->chunk_iters, costly, pull, l.F, l.prevF, l.pull_min, s.hist.hint[hp], l.it);
        const int pcap = persist_capacity(e);
        const bool resident = pull && n >= 2 && !s.trace && pcap > 0 && ep.n_groups > 0 && ep.n_groups <= pcap && resident_arena(e, ep);
        n = single_chunk_for_form(n, resident, pull, s.hist, hp, l.it, l.follow, e->chunk_iters, e->chunk_explicit);
        if (!pull && (rc = l.need_list())) return rc;
        if (resident) rc = l.resident_run(n); // (a failed roll-call: the same frontier again, now one launch per iteration)
        else if (!(rc = l.enqueue_chunk(n, pull, costly))) rc = l.finish_chunk(n, pull, costly);
        if (rc) return rc;
    }
    s.hist.record(hp, l.active_iters);
    if (l.form.must_zero_x()) { // leave both dense vectors all-zero for the next loop
        // only internal ids below n_int are ever written
        HIP_TRY(hipMemsetAsync(s.x, 0, sizeof(double) * (size_t)ep.grp_n_int, e->stream));
        HIP_TRY(hipMemsetAsync(s.x2, 0, sizeof(double) * (size_t)ep.grp_n_int, e->stream));
    }
    return DPPR_OK;
}

// ---------------------------------------------------------------------------------------------
// Both frontier loops of one batch as ONE resident launch, without a read-back in between.
//
// When consecutive batches behave alike (both phases start with a frontier worth a sweep -- the
// steady state of a sliding-window stream), the host knows what it will launch before it has seen
// any count. After a converged solve the frontier of a phase is {v : legal(residual[v])}, which the
// resident kernel reads off its registers (PLAN_SEED), and when phase 0 is over it seeds phase 1
// the same way and goes on (PLAN_BOTH): Inspect / snapshot / phase 0 / Inspect / snapshot / phase 1
// of gpu/PPRGPU.cuh:138-164 are one kernel. One copy of the counters, the status word and the log
// comes back at the end. Whatever did not go as expected (a phase needed more sweeps than the
// launch was given, the roll-call failed) leaves the state at a well-defined point from which the
// ordinary host-driven loop resumes (AheadOutcome::stage / entry).
// The reference pays a blocking read-back per ITERATION (gpu/PPRRevPushGPU.cuh:107).
// ---------------------------------------------------------------------------------------------
bool can_batch_ahead(const dppr_engine *e, const Slot &s, const Epoch &ep) {
    const int cap = persist_capacity(e);
    if (e->persist_mode != 1 || cap <= 0 || ep.n_groups <= 0 || ep.n_groups > cap || s.trace || e->chunk_iters <= 1 || ep.L <= 0)
        return false;
    // A resident sweep costs the same ~5 us whatever the frontier size, less than one push iteration's
    // launches: with the automatic push/pull threshold a window that can run resident always does.
    // With an explicit threshold (tests) only if the last batch's phases both started above it.
    if (e->merge_phases && e->schedule == DPPR_SCHEDULE_EAGER) // (the merged loop keeps its history in slot 0)
        return e->pull_min_frontier == 0 || (s.hist.hint[0] > 0 && s.start_dense[0]);
    return e->pull_min_frontier == 0 ||
           (s.hist.hint[0] > 0 && s.hist.hint[1] > 0 && s.start_dense[0] && s.start_dense[1]);
}

// What the launch reported comes back as `out` (AheadOutcome, dppr_loop_plan.hpp: decoded and applied to the slot there); a
// status other than DPPR_OK only for a HIP error or a wait that timed out inside the launch.
// merged (dppr_set_phase_merge): ONE loop over residuals of both signs -- the launch seeds it (PLAN_SEED) and runs it to the end
// (histories in slot 0); inline_update: the launch applies the batch's records itself (PLAN_UPDATE)
int batch_ahead(dppr_engine *e, Slot &s, const Epoch &ep, double eps, bool merged, bool inline_update, AheadOutcome &out) {
    const int n = batch_ahead_sweeps(merged, s.hist, e->chunk_iters, e->chunk_explicit);
    // (the launch's status word is s.cnt[7]; the GridBar was zeroed by the batch's first kernel, k_su_keys)
    const ResUpdate upd = !inline_update ? ResUpdate{}
                          : ep.grouped   ? ResUpdate{ep.su_rng, ep.sk, ep.sv, ep.b2, ep.ins, ep.deg_after, s.source, nullptr, 0}
                                         : ResUpdate{nullptr, nullptr, nullptr, ep.b2, ep.ins, nullptr, s.source, ep.b1, ep.L}; // raw records
    const int plan = (merged ? PLAN_SEED : (PLAN_SEED | PLAN_BOTH)) | (inline_update ? PLAN_UPDATE : 0);
    if (int rc = run_resident(e, s, ep, eps, 0, merged ? PHASE_BOTH : 0, n, plan, upd)) return rc;
    out = ahead_outcome(e->pinned[7], e->pinned[4], e->pinned[0], e->pinned + CNT_HDR, n, merged, inline_update, ep.grouped);
    s.st.persist_launches++;
    switch (out.kind) {
    case AHEAD_FAULT: return fail(e, DPPR_ERR_HIP, "a wait inside the resident sweep timed out");
    case AHEAD_CALLED_OFF_RECORDS: // not a residency problem: the caller applies the update with its own kernels, the next batches do so at once
        e->raw_backoff = 16;
        return DPPR_OK;
    case AHEAD_CALLED_OFF_ROLLCALL: // nothing was changed, the lists of the stream update stand; per-iteration launches for a while
        give_up_resident(e, s.st);
        return DPPR_OK;
    case AHEAD_RAN: break;
    }
    if (e->profiling)
        if (int rc = credit_launch(e, s.st, 0, false)) return rc;
    apply_ahead(out, merged, pull_min_frontier(e), s.hist, s.start_dense, s.last_F0, s.st.iterations, s.st.pull_iterations, s.st.sum_F);
    return DPPR_OK;
}

// full Inspect seeding + loop = ExecuteMainLoop(phase)
int main_loop_inspect(dppr_engine *e, Slot &s, const Epoch &ep, int phase, double eps) {
    s.seed_lists_valid = false;
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(int) * 3, e->stream));
    hipLaunchKernelGGL(k_inspect, dim3(grid_for(ep.grp_n_int, BLOCK * INSPECT_ITEMS)), dim3(BLOCK), 0, e->stream, s.r,
                       ep.grp_n_int, phase, eps, s.ft[0], s.cnt + 0);
    HIP_TRY(hipGetLastError());
    s.st.inspected += ep.grp_n_int;
    return run_frontier_loop(e, s, ep, phase, eps, 0, 0);
}

// The epoch's batch records grouped by tail (dppr_grouping.hpp): batch_tails = the tails, every tail ONE run (ascending tails
// for the at-slide, rank and radix paths; bucket by bucket for the bucket path), batch_order = the record indices, in batch
// order inside a run.
inline const uint32_t *batch_tails(const dppr_engine *e, const Epoch &ep) { return ep.grouped ? ep.sk : e->su_k[1]; }
inline const uint32_t *batch_order(const dppr_engine *e, const Epoch &ep) { return ep.grouped ? ep.sv : e->su_v[1]; }

// The grouping is a function of the batch's records alone (not of any solver state): by default it is done once, when the batch
// is uploaded (dppr_slide -> epoch_group_records; the reference uploads its GPUEdgeBatch untimed as well, gpu/PPRGPU.cuh:131-135),
// and the timed region starts with a kernel that only clears the loop's counters. dppr_set_batch_grouping(e, 0) keeps it inside
// dppr_update (the accounting of rounds 1-2: + 5 dispatches of the device radix sort per batch).
int epoch_group_records(dppr_engine *e, Epoch &ep) {
    ep.grouped = false;
    ep.su_inline = false;
    if (!e->group_at_slide || ep.L <= 0) return DPPR_OK;
    if (ep.id >= 0) { // an epoch built while the default accounting was on, grouped outside the bracket after all (prepare_epoch): its degrees too
        hipLaunchKernelGGL(k_copy_out_degree, dim3(grid_for(ep.L)), dim3(BLOCK), 0, e->bs, ep.b1, ep.L, ep.out_row_ptr, ep.deg_after);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_su_keys, dim3(grid_for(ep.L)), dim3(BLOCK), 0, e->bs, ep.b1, ep.L, e->su_k[0], e->su_v[0],
                       (unsigned long long *)nullptr, 0, (int *)nullptr, 0);
    size_t tmp = e->su_tmp_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(e->su_tmp.get(), tmp, e->su_k[0].get(), ep.sk.get(), e->su_v[0].get(), ep.sv.get(), (size_t)ep.L, 0u, (unsigned)e->bits, e->bs));
    ep.grouped = true;
    return res_record_ranges(e, ep);
}

inline GroupingPath in_region_path(const dppr_engine *e, const Epoch &ep) { return grouping_path(ep.L, ep.max_bucket, e->force_radix_grouping); }

// CopyOutDegree (gpu/StreamUpdate.cuh:7-17; a tail's post-batch out-degree = the length of its row in the epoch's out-CSR, written to
// `deg`) and the stable grouping of the L records by tail into su_k[1] / su_v[1], as the timed region runs them (`path` GROUPING_AUTO:
// in_region_path): ranked in one launch up to SU_RANK_MAX records, bucketed + ranked (three launches, dppr_update.hpp) up to
// SU_GRP_MAX_RECORDS unless one bucket would hold more than SU_GRP_MAX_BUCKET of them, the device radix sort otherwise. A test
// (dppr_debug_grouping) may name the path.
int enqueue_grouping(dppr_engine *e, const Epoch &ep, int *deg, unsigned long long *zero, int nz, int *zero_ints, int nzi,
                     GroupingPath path = GROUPING_AUTO) {
    const int L = ep.L;
    if (path == GROUPING_AUTO) path = in_region_path(e, ep);
    if (path == GROUPING_RANK) {
        hipLaunchKernelGGL(k_su_group_rank, dim3((L + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, e->stream, ep.b1, L, ep.out_row_ptr, e->su_k[1],
                           e->su_v[1], deg, zero, nz, zero_ints, nzi);
        HIP_TRY(hipGetLastError());
        return DPPR_OK;
    }
    if (path == GROUPING_BUCKET) {
        // hand-written: bucket histogram (+ CopyOutDegree + the counters), unordered scatter into the buckets, ranking inside them:
        // no library sort between the bracket's events
        const int nb = grouping_buckets(L);
        int *hist = e->su_grp, *cursor = hist + SU_GRP_MAX_BUCKETS, *ctl = cursor + SU_GRP_MAX_BUCKETS;
        const int wgs = (L + SU_GRP_PER_WG - 1) / SU_GRP_PER_WG;
        hipLaunchKernelGGL(k_su_grp_hist, dim3(wgs), dim3(BLOCK), 0, e->stream, ep.b1, L, nb, ep.out_row_ptr, deg, hist, zero, nz, zero_ints, nzi);
        hipLaunchKernelGGL(k_su_grp_scatter, dim3(wgs), dim3(BLOCK), 0, e->stream, ep.b1, L, nb, hist, cursor, ctl, e->su_k[0], e->su_v[0]);
        hipLaunchKernelGGL(k_su_grp_rank, dim3((L + BLOCK - 1) / BLOCK + nb), dim3(BLOCK), 0, e->stream, e->su_k[0], e->su_v[0], ctl, nb, e->su_k[1],
                           e->su_v[1], hist, cursor);
        HIP_TRY(hipGetLastError());
        return DPPR_OK;
    }
    // (batches beyond 4 Mi records or with a bucket above SU_GRP_MAX_BUCKET, or DPPR_GROUPING_RADIX=1: the device radix sort of rounds 1-5)
    hipLaunchKernelGGL(k_copy_out_degree, dim3(grid_for(L)), dim3(BLOCK), 0, e->stream, ep.b1, L, ep.out_row_ptr, deg);
    hipLaunchKernelGGL(k_su_keys, dim3(grid_for(L)), dim3(BLOCK), 0, e->stream, ep.b1, L, e->su_k[0], e->su_v[0], zero, nz, zero_ints, nzi);
    size_t tmp = e->su_tmp_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(e->su_tmp.get(), tmp, e->su_k[0].get(), e->su_k[1].get(), e->su_v[0].get(), e->su_v[1].get(), (size_t)L, 0u, (unsigned)e->bits, e->stream));
    return DPPR_OK;
}

int group_records_by_tail(dppr_engine *e, const Epoch &ep, unsigned long long *zero, int nz, int *zero_ints, int nzi) {
    if (ep.grouped) { // only the counters (and the GridBar of a resident launch enqueued ahead) are cleared here
        if (nz > 0 || nzi > 0)
            hipLaunchKernelGGL(k_su_keys, dim3(1), dim3(BLOCK), 0, e->stream, ep.b1, 0, e->su_k[0], e->su_v[0], zero, nz, zero_ints, nzi);
        HIP_TRY(hipGetLastError());
        return DPPR_OK;
    }
    return enqueue_grouping(e, ep, ep.deg_after, zero, nz, zero_ints, nzi); // inside the timed region (default)
}

// dppr_set_batch_grouping(1) after epochs were built: their records are grouped now, BEFORE the caller's event bracket opens
inline int prepare_epoch(dppr_engine *e, Epoch &ep) {
    if (e->group_at_slide && !ep.grouped && ep.L > 0) {
        if (int rc = epoch_group_records(e, ep)) return rc;
        HIP_TRY(hipStreamSynchronize(e->bs)); // (the grouping ran on the builder's stream; what follows reads it on the solver's)
    }
    return DPPR_OK;
}

int stream_update(dppr_engine *e, Slot &s, const Epoch &ep, double eps, bool seed, bool zero_bars = false) {
    const int L = ep.L;
    if (L == 0) {
        HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(int) * 5, e->stream));
        return DPPR_OK;
    }
    // (the batch's first kernel also clears cnt[0..4] and, for a resident launch enqueued ahead, its GridBar)
    int rc = group_records_by_tail(e, ep, zero_bars ? reinterpret_cast<unsigned long long *>(e->bar.get()) : nullptr,
                                   zero_bars ? (int)(sizeof(GridBar) / sizeof(unsigned long long)) : 0, s.cnt, 5);
    if (rc) return rc;
    // without seeding the lists go to scratch space (cnt[4] / neg) and are ignored
    if (L >= SU_SPLIT_MIN) {
        // Large batches: a hub's tail owns thousands of records, and the fused kernel's leader walks what lies beyond its
        // 1 024-record LDS window through three dependent gathers per record (twitter stand-in, 2.9 M records: 3.0 ms of a batch).
        // The terms of ALL records are computed in parallel first; the leaders then walk contiguous arrays (same expressions,
        // same order: bit-identical, the form source groups use).
        SuSources srcs{};
        srcs.s[0] = s.source;
        hipLaunchKernelGGL(k_su_terms, dim3(grid_for(L), 1), dim3(BLOCK), 0, e->stream, batch_tails(e, ep), batch_order(e, ep), ep.b2, ep.ins, L, s.p, 1,
                           e->su_term, e->su_ins);
        hipLaunchKernelGGL(k_su_apply, dim3(grid_for(L), 1), dim3(BLOCK), 0, e->stream, batch_tails(e, ep), batch_order(e, ep), e->su_term, e->su_ins,
                           ep.deg_after, L, s.r, 1, srcs, seed ? eps : 1e300, s.ft[0], s.cnt + 0, s.neg, s.cnt + 3);
    } else {
        hipLaunchKernelGGL(k_su_apply_fused, dim3(grid_for(L)), dim3(BLOCK), 0, e->stream, batch_tails(e, ep), batch_order(e, ep), ep.b2, ep.ins,
                           ep.deg_after, L, s.p, s.r, s.source, seed ? eps : 1e300, s.ft[0], s.cnt + 0, s.neg, s.cnt + 3);
    }
    HIP_TRY(hipGetLastError());
    s.st.records += L;
    return DPPR_OK;
}

// the edge counts the kernels keep (of a slot or of a source group), and what follows from the counters: one place for both
int pull_device_stats(dppr_engine *e, const IterStats *dstats, dppr_stats_t &st) {
    static thread_local IterStats h[2];
    HIP_TRY(hipMemcpyAsync(h, dstats, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long t = 0, ts = 0;
    for (int i = 0; i < STAT_SLOTS; ++i) {
        t += h[0].blk_E[i];
        ts += h[1].blk_E[i];
    }
    st.sum_E = (int64_t)(t + ts);
    st.sweep_E = (int64_t)ts;
    // every enqueued vertex is a frontier member of a later iteration, except the seeds
    st.sum_N = st.sum_F;
    // SURVEY.md 8(d); its Inspect term (8 bytes per vertex and pass) is counted for the passes that RAN:
    // after a converged solve the frontier is seeded from the batch tails and no vertex is scanned
    st.algorithmic_bytes = 8ll * st.inspected + 45ll * st.records + 72ll * st.sum_F + 24ll * st.sum_E + 4ll * st.sum_N;
    return DPPR_OK;
}

// dppr_stats / dppr_group_stats and their resets
int solve_stats(dppr_engine *e, SolveState &o, dppr_stats_t *out) {
    if (int rc = pull_device_stats(e, o.dstats, o.st)) return rc;
    *out = o.st;
    return DPPR_OK;
}
int solve_reset_stats(dppr_engine *e, SolveState &o) {
    o.st = dppr_stats_t{};
    HIP_TRY(hipMemsetAsync(o.dstats, 0, 2 * sizeof(IterStats), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return DPPR_OK;
}

// the candidates the update recorded below -eps (s.neg, cnt[3]), re-checked now, appended to the list in ft[0] / cnt[0]
// (clear: after cnt[0..2] were zeroed -- the list then holds them alone)
int filter_negative_tails(dppr_engine *e, Slot &s, const Epoch &ep, double eps, bool clear) {
    if (clear) HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(int) * 3, e->stream));
    hipLaunchKernelGGL(k_filter, dim3(grid_for(std::max(ep.L, 1))), dim3(BLOCK), 0, e->stream, s.neg, s.cnt + 3, s.r, 1, eps, s.ft[0], s.cnt + 0);
    HIP_TRY(hipGetLastError());
    return DPPR_OK;
}

// One batch of one source = dppr_update: IncrementalBatchUpdate and both frontier loops (gpu/PPRGPU.cuh:138-164), inside the
// event bracket. Top to bottom: settle, prepare, open the bracket; the update (or, where a whole-batch launch applies it, the
// kernel that clears the counters); that launch; after_launch (dppr_loop_plan.hpp) says what follows; at most one redone update,
// one filter and two loops; close the bracket.
int slot_update(dppr_engine *e, Slot &s, Epoch &ep, double eps, float *out_ms) {
    if (!e->persist_ok && e->persist_mode && e->persist_retry > 0 && --e->persist_retry == 0)
        e->persist_ok = true; // a resident launch gave up a while ago (the CUs were shared): try them again
    s.seed_lists_valid = false;
    // Seeding from the batch tails is exact only if every |r| <= eps beforehand
    // (the state a completed solve leaves). Otherwise fall back to full Inspect passes.
    // Merged loop (dppr_set_phase_merge, eager schedule): residuals of both signs are pushed in ONE loop, to eps / merge_div.
    const bool merged = e->merge_phases && e->schedule == DPPR_SCHEDULE_EAGER;
    if (merged) eps = eps / e->merge_div;
    const bool seeded = s.converged && s.conv_eps <= eps;
    const bool ahead = seeded && can_batch_ahead(e, s, ep) && resident_arena(e, ep);
    int rc = settle_parked(e, s.p, s.r, 1, eps, &s.park_eps, &s.st);
    if (rc) return rc;
    rc = prepare_epoch(e, ep);
    if (rc) return rc;
    if (e->raw_backoff > 0) --e->raw_backoff;
    rc = bracket_open(e);
    if (rc) return rc;
    // A whole-batch resident launch applies the records itself (PLAN_UPDATE) -- grouped at slide time and cut into the sweep groups'
    // ranges, or (default accounting) RAW: the launch finds, orders and applies every group's records itself. Only the counters
    // and the GridBar are cleared here. Should the launch call itself off, nothing was changed and the update runs as its own
    // kernels after all.
    const bool raw_ok = !ep.grouped && ep.L > 0 && ep.L <= RES_RAW_STEPS * sweep_block(e) && e->raw_backoff == 0;
    const bool inline_su = ahead && e->res_update && ((ep.su_inline && ep.grouped) || raw_ok);
    if (inline_su) {
        hipLaunchKernelGGL(k_su_keys, dim3(1), dim3(BLOCK), 0, e->stream, ep.b1, 0, e->su_k[0], e->su_v[0],
                           reinterpret_cast<unsigned long long *>(e->bar.get()), (int)(sizeof(GridBar) / sizeof(unsigned long long)), s.cnt, 5);
        HIP_TRY(hipGetLastError());
    } else {
        rc = stream_update(e, s, ep, eps, seeded, ahead);
    }
    if (rc) return rc;
    s.converged = false;
    AheadOutcome launched; // (no launch: as constructed)
    if (ahead && (rc = batch_ahead(e, s, ep, eps, merged, inline_su, launched))) return rc;
    const AfterLaunch then = after_launch(merged, seeded, ahead, inline_su, launched);
    if (then.redo_update && (rc = stream_update(e, s, ep, eps, seeded, false))) return rc;
    if (then.count_records) s.st.records += ep.L;
    for (int k = 0; k < then.n_loops; ++k) {
        const LoopStep &l = then.loop[k];
        if (then.filter && k == then.n_loops - 1 && (rc = filter_negative_tails(e, s, ep, eps, then.filter_clears))) return rc;
        rc = l.inspect ? main_loop_inspect(e, s, ep, l.phase, eps) : run_frontier_loop(e, s, ep, l.phase, eps, 0, 0, l.entry);
        if (rc) return rc;
    }
    return solve_finished(e, s, eps, ep.id, true, out_ms); // (eps: the merged loop's eps / merge_div)
}

} // namespace
