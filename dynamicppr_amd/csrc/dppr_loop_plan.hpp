// dppr_loop_plan.hpp -- the POLICY of the frontier loops: how many sweeps to enqueue before the next read-back, what a resident or
// multi-sweep launch is given, when a group's push tail takes over and at what threshold, push or sweep by estimated cost, and the
// loop histories all of that is sized from -- and, one layer above the loops, what a whole-batch launch of a single source
// reported (AheadOutcome) and what a batch therefore runs after it (AfterLaunch) -- and which representation of a single-source
// loop's frontier is live, list or dense snapshot (FrontierForm). Pure functions of plain integers, without HIP
// includes: run_frontier_loop / batch_ahead / slot_update (dppr_host_loop.hpp) and group_loop / group_push_tail
// (dppr_host_group.hpp) ask here, launch, read back and account; tests/native/loop_plan_test.cpp drives every function on the CPU
// against a plain restatement, and replays whole loops.
#pragma once

#include <algorithm>
#include <cstdint>

namespace dppr {

constexpr int MAX_CHUNK = 64;              // one-launch-per-iteration chunks: iterations enqueued between two read-backs at most
constexpr int GMULTI_MAX = 2 * MAX_CHUNK;  // sweeps a multi-sweep launch of a source group may run
constexpr int RESIDENT_MARGIN = 8;         // sweeps a resident launch is given beyond what the last batch needed
// what the kernels' headers fix (asserted equal in dppr_engine.hip: RES_MAX_SWEEPS of dppr_resident.hpp, GPUSH_LOG / TINY_N / TINY_E
// of dppr_gpush.hpp)
constexpr int PLAN_RES_MAX_SWEEPS = 128;   // sweeps of one resident launch at most
constexpr int PLAN_GPUSH_LOG = 16;         // iterations one chunk of a group's push tail may hold
constexpr int PLAN_TINY_N = 512, PLAN_TINY_E = 1024; // vertices / in-edges the single-workgroup form of the push tail takes
// status word of a resident launch (k_pull_resident, dppr_resident.hpp, writes it; ahead_outcome below and run_frontier_loop read it)
constexpr int PERSIST_ABORTED = 1 << 30;   // the roll-call failed, nothing was changed
constexpr int PERSIST_FAULT = 1 << 29;     // a wait timed out after a successful roll-call
constexpr int PERSIST_CONVERGED = 1 << 28; // the frontier emptied; all snapshot vectors are all zero again
constexpr int PERSIST_PHASE1 = 1 << 26;    // a launch that runs both phases had started phase 1
constexpr int PERSIST_SWEEPS = (1 << 16) - 1; // low bits: loop position g
constexpr int LOOP_PHASE_BOTH = 2;         // the merged loop's phase (asserted equal to PHASE_BOTH of dppr_common.hpp in dppr_engine.hip)

// ---------------------------------------------------------------------------- loop histories
// What the last loops of each phase took (the merged loop uses slot 0): consecutive batches take about the same number of
// iterations, so the next loop's chunks are sized from them.
struct LoopHistory {
    int hint[2] = {0, 0};                             // iterations the last loop of each phase took
    int hist[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};    // ... and the last four
    int dense[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};   // source groups: sweeps before the frontier was small enough for the push form

    void record(int hp, int iters) {
        hint[hp] = iters;
        push(hist[hp], iters);
    }
    void record_dense(int hp, int len) { push(dense[hp], len); }
    // the SHORTEST of the last four loops (0: no history yet): a first chunk of that length is almost surely needed in full
    int shortest(int hp) const { return least(hist[hp]); }
    int shortest_dense(int hp) const { return least(dense[hp]); }

  private:
    static void push(int (&row)[4], int v) {
        for (int k = 3; k > 0; --k) row[k] = row[k - 1];
        row[0] = v;
    }
    static int least(const int (&row)[4]) {
        int lo = 0;
        for (int h : row) lo = h > 0 && (lo == 0 || h < lo) ? h : lo;
        return lo;
    }
};

// a follow-up chunk of one-launch-per-iteration sweeps, each twice as long as the one before up to chunk_iters. (The doubling
// stops at 2^30, far above any chunk_iters: a loop of more than thirty such chunks used to overflow the int.)
inline int follow_up_chunk(int &follow, int chunk_iters) {
    const int n = std::min(follow, chunk_iters);
    if (follow < (1 << 30)) follow *= 2;
    return n;
}

// ---------------------------------------------------------------------------- source groups (group_loop, group_push_tail)
// the tail of a group's loop runs as pushes (dppr_gpush.hpp) below this many frontier pairs; 0: never.
// enter_pairs: dppr_set_group_push (-1: automatic, auto_factor pairs per sweep group)
inline long long group_push_threshold(int enter_pairs, int n_ggroups, int auto_factor) {
    return enter_pairs == 0 ? 0 : enter_pairs > 0 ? enter_pairs : std::max(64, n_ggroups * auto_factor);
}

// sweeps a multi-sweep launch is given at loop position `it` (a window whose sweep groups are all resident at once)
inline int group_multi_sweeps(int hint, int it, int chunk_iters, bool chunk_explicit) {
    int n = hint > it ? hint - it + RESIDENT_MARGIN : 2 * chunk_iters;
    n = std::max(2, std::min(n, GMULTI_MAX));
    if (chunk_explicit) n = std::min(n, std::max(chunk_iters, 2)); // (tests: launches that stop mid-loop and are resumed)
    return n;
}

// what one loop of a group carries from chunk to chunk
struct GroupLoopPlan {
    int follow = 4;            // size of the next follow-up chunk of one-sweep launches
    long long push_thr = 0;    // the push form takes over at this many frontier pairs (0: never)
    bool push_gave_up = false; // the push form is not tried again in this loop
    int dense_len = -1;        // sweeps of this loop before the frontier was that small (-1: it never was)

    // One-sweep launches are enqueued in chunks; a launch that finds every frontier empty returns at once, but it
    // still costs a dispatch (~4 us + gap). Consecutive batches take about the same number of sweeps, so the first
    // chunk is the SHORTEST of the last four loops of this phase (almost surely needed in full), and what follows
    // doubles from 4: a boundary (read-back + relaunch) costs about three empty dispatches.
    // F: the live frontier's pairs as the last read-back showed them.
    int next_chunk(const LoopHistory &h, int hp, int it, long long F, int chunk_iters, bool chunk_explicit) {
        int n;
        if (it == 0) {
            const int lo = push_thr > 0 ? h.shortest_dense(hp) : h.shortest(hp);
            n = lo > 0 ? lo : chunk_iters;
            follow = 4;
        } else if (push_thr > 0 && !push_gave_up) {
            // the push form takes over below push_thr pairs and a sweep of the tail costs its floor whatever it finds: go
            // only as far as the frontier is sure to stay above the threshold (it shrinks by <= ~4x per sweep down there)
            n = 1;
            for (long long f = F / 4; f > push_thr && n < chunk_iters; f /= 4) ++n;
        } else {
            n = follow_up_chunk(follow, chunk_iters);
        }
        if (chunk_explicit) n = std::min(n, std::max(chunk_iters, 1));
        return std::max(1, std::min(n, MAX_CHUNK));
    }
    // sweep `at` of the loop FOUND a frontier of F pairs (that sweep could have been a push iteration if F is this small)
    void saw_frontier(long long F, int at) {
        if (push_thr > 0 && dense_len < 0 && F <= push_thr) dense_len = at;
    }
    // a chunk is over with F pairs left: hand the tail to the push form now?
    bool enter_push(bool more, long long F) const { return more && push_thr > 0 && !push_gave_up && F <= push_thr; }
    // the push form gave the frontier back (an iteration too large for it) or did not take it (it did not fit the lists):
    // the next try waits for a much smaller frontier
    void push_declined(long long F) {
        push_thr = std::max<long long>(F / 8, 1);
        dense_len = -1;
    }
    // the loop is over after active_iters iterations
    void finish(LoopHistory &h, int hp, int active_iters) const {
        if (push_thr > 0) h.record_dense(hp, dense_len >= 0 ? std::max(dense_len, 1) : std::max(active_iters, 1));
        h.record(hp, active_iters);
    }
};

// in-edges one iteration of the push tail may have (configured: dppr_set_group_push, 0 = from the sweep's floor).
// what an iteration may cost here: a sweep's floor is ~0.02 us per sweep group, a returning f64 atomic ~1 / 20 000 us
// (round 6: 20 in-edges per sweep group, was 200 -- on the headline's 3 075 groups a push iteration of up to 615 K in-edges x 10 sources cost up
// to 540 us where a near-empty sweep costs 50-85: bound 615 K / 150 K / 60 K / 40 K / 20 K -> 12.37 / 12.24 / 12.18 / 12.19 / 12.23 ms per batch,
// two runs each on one box; twitter / friendster groups and resident-size windows: unchanged)
inline long long gpush_edge_bound(long long configured, int n_ggroups) {
    return configured > 0 ? configured : std::max<long long>(4096, 20ll * std::max(n_ggroups, 1));
}

// iterations per chunk of the three-kernel form (<= GPUSH_LOG): down here the frontier about halves per iteration, so the first
// chunk is sized to reach the single-workgroup form (an iteration that finds nothing is three empty dispatches)
inline int gpush_chunk(int it_done, long long pairs_at_entry) {
    int m = 2;
    if (it_done == 0)
        for (long long f = pairs_at_entry; f > 128 && m < PLAN_GPUSH_LOG; f >>= 2) ++m;
    return m;
}

// edge x source adds of the last iteration as far as they are known on the way in (-1: not known yet)
inline long long gpush_adds_at_entry(long long pairs_at_entry) { return pairs_at_entry <= 64 ? 0 : -1; }

// a frontier of a few hundred vertices: a run of iterations as ONE single-workgroup launch (known_n: the frontier's vertices, or an
// upper bound of them; last_adds: edge x source adds of the last iteration run, -1 = not known yet)
inline bool gpush_take_tiny(long long known_n, long long last_adds, bool tiny_declined) {
    return known_n <= PLAN_TINY_N && last_adds >= 0 && last_adds <= PLAN_TINY_E / 2 && !tiny_declined;
}
// a chunk ran no iteration without calling the mode off: too many vertices or in-edges for one workgroup
inline bool gpush_tiny_declined(bool progressed, bool stopped, long long known_n) { return !progressed && !stopped && known_n <= PLAN_TINY_N; }

// ---------------------------------------------------------------------------- single source (run_frontier_loop, batch_ahead)
constexpr int PULL_NEVER = 0x7fffffff;
// frontier size from which an iteration is a sweep (setting: dppr_set_tuning; 0 = automatic, < 0 = never)
inline int pull_min_frontier(int setting, int Ed) { return setting > 0 ? setting : setting < 0 ? PULL_NEVER : std::max(1024, Ed / 192); }

// what a sweep of a window of Ed edges costs, in microseconds (mean_us: the running mean of this slot's sweeps, 0 = none timed yet:
// ~6.5 ps per edge)
inline double sweep_cost_us(double mean_us, int Ed) { return mean_us > 0 ? mean_us : 6.5e-6 * (double)Ed; }
// a window whose iterations cost hundreds of microseconds and more (twitter / friendster size): decisions per iteration
inline bool window_costly(bool binned, bool chunk_explicit, double mean_us, int Ed) {
    return binned && !chunk_explicit && sweep_cost_us(mean_us, Ed) >= 300.0;
}

// Push or sweep by what each would cost. A push is one returning atomic per in-edge of the
// frontier, executed at the memory side at ~23.5 G/s chip-wide whatever the locality (profiles/r03_atomics_probe.json);
// a sweep of this window costs what the last ones did. The frontier's in-edges are counted by the sweep that left it
// (k_bin_reduce) or, for a list, by k_front_degree. (Round 3 switched on the vertex count: a late frontier of 1.7 M
// low-degree vertices is pushed in 0.23 ms and was swept for 2.6, the 156 K batch tails -- hubs -- cost a sweep's time.)
constexpr int COST_MIN_FRONTIER = 1024; // smaller frontiers are pushed unpriced
// D: in-edges of the frontier, -1 = not counted
inline bool cost_needs_degrees(int F, long long D) { return D < 0 && F >= COST_MIN_FRONTIER; }
inline bool cost_decides(int F, long long D) { return D >= 0 || F < COST_MIN_FRONTIER; }
inline bool cost_says_sweep(int F, long long D, double mean_sweep_us, int Ed, double atomic_ns) {
    const double sweep_us = sweep_cost_us(mean_sweep_us, Ed);
    const double push_us = 15.0 + (double)std::max<long long>(D, 0) * atomic_ns * 1e-3; // (measured on this slot's own pushes)
    return F >= COST_MIN_FRONTIER && push_us > 0.9 * sweep_us;
}
// the two running means behind it, after an iteration that ran alone between two events: what a sweep of this window costs ...
inline double mean_sweep_us(double old_us, float ms) { return old_us > 0 ? 0.75 * old_us + 0.25 * ms * 1e3 : ms * 1e3; }
// ... and what an atomic of a push does (pushes of fewer than 2^20 in-edges say nothing about it)
inline double mean_atomic_ns(double old_ns, float ms, long long D) {
    return D >= (1 << 20) ? 0.75 * old_ns + 0.25 * std::min(1.0, std::max(0.02, (ms * 1e6 - 15e3) / (double)D)) : old_ns;
}

// iterations of the next chunk, before the launch form is known. F / prevF: this frontier's size and the one before it
inline int single_chunk(bool trace, int chunk_iters, bool costly, bool pull, int F, int prevF, int pull_min, int hint, int it) {
    if (trace || chunk_iters <= 1) return 1;
    if (costly)
        // A window on binned sweeps: an iteration costs milliseconds (friendster stand-in: 2.6 ms a sweep, 11-13 ms the push
        // of a 3-10 M-vertex frontier), a read-back tens of microseconds. Nothing is enqueued blind: round 3 ran the second
        // iteration of every loop as a push of ten million vertices (decided at 156 K) and ended every loop with three to
        // seven sweeps over frontiers of a few hundred vertices (enqueued from the last batches' lengths) -- 40 of 183 ms.
        return (!pull && F < 4096 && F <= prevF) ? chunk_iters : 1;
    if (pull) return hint > it ? hint - it + 1 : chunk_iters; // consecutive batches take almost the same number of iterations: aim just past the end
    if ((long long)F * 4 >= pull_min) return 1;               // about to turn dense: re-decide next iteration
    return F > prevF ? 2 : chunk_iters;                       // growing: short chunks; decaying tail: long
}
// ... and once it is: `resident` = the chunk runs as ONE resident launch. follow: size of the next follow-up chunk of per-iteration
// sweeps, 4 when a loop starts
inline int single_chunk_for_form(int n, bool resident, bool pull, const LoopHistory &h, int hp, int it, int &follow, int chunk_iters,
                                 bool chunk_explicit) {
    if (resident && h.hint[hp] > it) n += RESIDENT_MARGIN - 1;
    if (!resident && pull && n > 1) {
        // per-iteration sweeps: a launch that finds the frontier empty is still a dispatch, a chunk boundary (read-back
        // + relaunch) costs about three of them -- go as far as the SHORTEST of the last four loops of this phase went
        // (almost surely needed in full), then in chunks that double from 4 (group_loop sizes its chunks the same way)
        const int lo = h.shortest(hp);
        if (lo > it) n = lo - it;
        else if (lo > 0) n = follow_up_chunk(follow, chunk_iters);
    }
    n = std::min(n, MAX_CHUNK);
    if (chunk_explicit) n = std::min(n, std::max(chunk_iters, 1));
    return resident ? std::min(n, PLAN_RES_MAX_SWEEPS) : n;
}

// sweeps a whole-batch resident launch (batch_ahead) is given. A resident launch stops by itself when the frontier empties: a
// generous allowance costs nothing, a short one costs a read-back and another launch (+1: the step that seeds phase 1)
inline int batch_ahead_sweeps(bool merged, const LoopHistory &h, int chunk_iters, bool chunk_explicit) {
    int n = merged ? (h.hint[0] > 0 ? std::min(h.hint[0] + 2 * RESIDENT_MARGIN, 2 * MAX_CHUNK) : 2 * MAX_CHUNK)
            : h.hint[0] > 0 && h.hint[1] > 0 ? std::min(h.hint[0] + h.hint[1] + 1 + 2 * RESIDENT_MARGIN, 2 * MAX_CHUNK)
                                             : 2 * MAX_CHUNK; // no history yet
    if (chunk_explicit) n = std::min(n, chunk_iters); // (tests: launches that stop mid-phase and are resumed)
    return std::min(n, PLAN_RES_MAX_SWEEPS);
}

// the log of such a launch: frontier sizes of phase 0, a zero (phase 0 over), those of phase 1, a zero. `entries`: what the
// launch wrote of it
struct PhaseLog {
    int act[2] = {0, 0};   // sweeps of each phase that saw a frontier
    int F0[2] = {0, 0};    // ... the first of those frontiers (valid where act > 0)
    long long sum_F = 0;   // all frontiers together
};
inline PhaseLog split_phase_log(const int *log, int entries) {
    PhaseLog pl;
    for (int k = 0, ph = 0; k < entries && ph < 2; ++k) {
        if (log[k] <= 0) {
            ++ph;
            continue;
        }
        if (pl.act[ph] == 0) pl.F0[ph] = log[k];
        pl.sum_F += log[k];
        pl.act[ph]++;
    }
    return pl;
}

// ---------------------------------------------------------------------------- a whole batch of a single source (batch_ahead, slot_update)
// a frontier loop that is picked up in the middle (after a launch of batch_ahead that ended before the loop did): iterations
// already done, the frontier size if the host knows it, and whether the slot's x already holds the frontier's dense snapshot
struct LoopEntry {
    int it = 0;
    int F = -1; // -1: read cnt[cur]
    bool dense = false;
    bool any_pull = false;
};

// Which representation of a single-source loop's frontier is live (run_frontier_loop): the list in s.ft[buf], the dense snapshot
// in s.x, or both -- never neither. Every launch of the loop is one transition; the loop asks before it enqueues.
struct FrontierForm {
    bool list;              // s.ft[buf] holds the frontier as a list (sweeps only count it)
    bool dense;             // s.x holds the snapshot of the current frontier (p already updated)
    bool extracted = false; // ... and that snapshot zeroed the residuals it took (InspectExtra): the push needs no repair
    bool any_pull;          // a sweep ran: s.x / s.x2 are no longer all zero
    bool x_clean = false;   // a resident launch ended the loop and left s.x / s.x2 all zero

    explicit FrontierForm(const LoopEntry &en) : list(!en.dense), dense(en.dense), any_pull(en.any_pull) {}
    void list_made() { list = true; }                                // k_list_from_dense: the snapshot as a list
    void snapshot_taken(bool extr) { dense = true, extracted = extr; } // k_snapshot_dense: the list as a snapshot
    void pushed() { dense = extracted = false, list = true; }        // a push iteration consumed (and zeroed) the snapshot, wrote a list
    void swept() { dense = any_pull = true, extracted = list = false; } // a per-iteration sweep wrote the next snapshot, counted the list
    void resident_returned(bool converged) { list = false, any_pull = true, x_clean = converged; } // (the last sweep's snapshot is in s.x)

    bool needs_list() const { return !list; }         // before a push or a trace copy
    bool needs_snapshot() const { return !dense; }    // before a sweep or a synchronous push
    bool must_zero_x() const { return any_pull && !x_clean; } // at the end: leave both dense vectors all zero for the next loop
};

// What a whole-batch resident launch reported. A launch that was CALLED OFF changed nothing: a sweep group owned more of the raw
// records than it has threads (RECORDS: not a residency problem), or the roll-call failed (ROLLCALL: the grid was not co-resident).
enum AheadKind { AHEAD_FAULT, AHEAD_CALLED_OFF_RECORDS, AHEAD_CALLED_OFF_ROLLCALL, AHEAD_RAN };
struct AheadOutcome {
    AheadKind kind = AHEAD_RAN;
    int stage = 0;          // 0: phase 0 (the merged loop) still open, 1: phase 0 done and phase 1 open, 2: the batch is done
    bool p1_seeded = false; // phase 1's snapshot exists (the launch seeded it)
    LoopEntry entry;        // where the open loop of `stage` resumes (as constructed: from its start)
    PhaseLog log;           // what the launch's log says of each phase
    bool called_off() const { return kind == AHEAD_CALLED_OFF_RECORDS || kind == AHEAD_CALLED_OFF_ROLLCALL; }
};
// status, cnt4, cnt0: words 7 (status word), 4 (1: a group owns too many records) and 0 (the live frontier size) of the counters
// the launch left; log: its n entries; merged / inline_update: the launch's plan; grouped: the records it took were grouped at slide
inline AheadOutcome ahead_outcome(int status, int cnt4, int cnt0, const int *log, int n, bool merged, bool inline_update, bool grouped) {
    AheadOutcome o;
    if (status & PERSIST_FAULT) o.kind = AHEAD_FAULT;
    else if (status & PERSIST_ABORTED) o.kind = inline_update && !grouped && cnt4 == 1 ? AHEAD_CALLED_OFF_RECORDS : AHEAD_CALLED_OFF_ROLLCALL;
    if (o.kind != AHEAD_RAN) return o;
    const int pos = status & PERSIST_SWEEPS; // loop position the launch stopped at
    o.log = split_phase_log(log, std::min(pos + 1, n));
    const bool phase0_done = merged ? (status & PERSIST_CONVERGED) != 0 : (status & PERSIST_PHASE1) != 0;
    o.stage = !phase0_done ? 0 : merged || (status & PERSIST_CONVERGED) ? 2 : 1;
    o.p1_seeded = !merged && phase0_done;
    if (o.stage < 2) o.entry = LoopEntry{o.log.act[o.stage], cnt0, true, true}; // out of sweeps: the host-driven loop goes on from here
    return o;
}
// ... and what a launch that RAN leaves in the slot: the first frontiers of the phases it saw, the iterations it ran, and the
// histories of the loops it finished. The merged loop records through LoopHistory::record (which also pushes the ring that
// shortest() reads); the two phases write hint[] alone and leave the ring to the host-driven loops. That asymmetry is deliberate
// to the refactor that moved these lines here: unchanged, not judged.
inline void apply_ahead(const AheadOutcome &o, bool merged, int pull_min, LoopHistory &hist, bool (&start_dense)[2], int (&last_F0)[2],
                        int64_t &iterations, int64_t &pull_iterations, int64_t &sum_F) {
    if (o.kind != AHEAD_RAN) return;
    const int *act = o.log.act;
    for (int ph = 0; ph < 2; ++ph)
        if (act[ph] > 0) {
            start_dense[ph] = o.log.F0[ph] >= pull_min;
            last_F0[ph] = o.log.F0[ph];
        }
    iterations += act[0] + act[1];
    pull_iterations += act[0] + act[1];
    sum_F += o.log.sum_F;
    const int finished = merged ? o.stage / 2 : o.stage; // loops the launch ran to their end
    for (int ph = 0; ph < finished; ++ph) {
        if (merged) hist.record(0, act[0]);
        else hist.hint[ph] = act[ph];
        if (act[ph] == 0) start_dense[ph] = false;
    }
}

// What a batch runs after its update (and after the whole-batch launch, if one was made). merged / seeded / ahead / inline_su: the
// batch runs the merged loop / starts from a converged state (frontiers from the batch's tails) / made a whole-batch launch / that
// launch was to apply the records itself; o: what it reported (as constructed where none was made).
struct LoopStep {
    int phase = 0;        // 0, 1 or LOOP_PHASE_BOTH
    bool inspect = false; // seed by a full Inspect pass; otherwise enter at `entry`
    LoopEntry entry;
};
struct AfterLaunch {
    bool redo_update = false;   // the launch called itself off: the update runs as its own kernels after all ...
    bool count_records = false; // ... or it applied the records: they are counted
    bool filter = false;        // the update's candidates below -eps join (merged) or become (phase 1) the list the LAST loop starts from
    bool filter_clears = false; // ... after cnt[0..2] were cleared (phase 1: phase 0 used them)
    int n_loops = 0;
    LoopStep loop[2];
};
inline AfterLaunch after_launch(bool merged, bool seeded, bool ahead, bool inline_su, const AheadOutcome &o) {
    AfterLaunch d;
    auto add = [&d](int phase, bool inspect, LoopEntry entry = LoopEntry()) { d.loop[d.n_loops++] = LoopStep{phase, inspect, entry}; };
    if (ahead && o.kind == AHEAD_FAULT) return d; // (batch_ahead returned the error)
    if (ahead && inline_su) {
        d.redo_update = o.called_off();
        d.count_records = !d.redo_update;
        inline_su = !d.redo_update;
    }
    if (merged) {
        if (!seeded) add(LOOP_PHASE_BOTH, true);
        else if (!ahead || o.stage != 2) {
            // the frontier: the tails the update left above eps (ft[0]) and those it left below -eps (the candidates). A launch
            // that ran out of sweeps left a dense snapshot; one that was called off left the update's lists standing
            d.filter = !ahead || (o.entry.it == 0 && !o.entry.dense);
            add(LOOP_PHASE_BOTH, false, ahead ? o.entry : LoopEntry());
        }
        return d;
    }
    if (!seeded) {
        add(0, true);
        add(1, true);
        return d;
    }
    const int stage = ahead ? o.stage : 0;
    if (stage == 0) add(0, false, ahead ? o.entry : LoopEntry());
    if (stage <= 1) {
        const bool p1_seeded = ahead && o.p1_seeded;
        // the update ran inside the launch and recorded no candidates: phase 1 starts from a full Inspect; otherwise from the
        // candidates the update recorded, re-checked now
        if (!p1_seeded && inline_su) add(1, true);
        else {
            d.filter = d.filter_clears = !p1_seeded;
            add(1, false, stage == 1 ? o.entry : LoopEntry());
        }
    }
    return d;
}

} // namespace dppr
