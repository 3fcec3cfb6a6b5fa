// dppr_loop_plan.hpp -- the POLICY of the frontier loops: how many sweeps to enqueue before the next read-back, what a resident or
// multi-sweep launch is given, when a group's push tail takes over and at what threshold, push or sweep by estimated cost, and the
// loop histories all of that is sized from. Pure functions of plain integers, without HIP includes: run_frontier_loop / batch_ahead
// (dppr_host_loop.hpp) and group_loop / group_push_tail (dppr_host_group.hpp) ask here, launch, read back and account;
// tests/native/loop_plan_test.cpp drives every function on the CPU against a plain restatement, and replays whole loops.
#pragma once

#include <algorithm>

namespace dppr {

constexpr int MAX_CHUNK = 64;              // one-launch-per-iteration chunks: iterations enqueued between two read-backs at most
constexpr int GMULTI_MAX = 2 * MAX_CHUNK;  // sweeps a multi-sweep launch of a source group may run
constexpr int RESIDENT_MARGIN = 8;         // sweeps a resident launch is given beyond what the last batch needed
// what the kernels' headers fix (asserted equal in dppr_engine.hip: RES_MAX_SWEEPS of dppr_resident.hpp, GPUSH_LOG / TINY_N / TINY_E
// of dppr_gpush.hpp)
constexpr int PLAN_RES_MAX_SWEEPS = 128;   // sweeps of one resident launch at most
constexpr int PLAN_GPUSH_LOG = 16;         // iterations one chunk of a group's push tail may hold
constexpr int PLAN_TINY_N = 512, PLAN_TINY_E = 1024; // vertices / in-edges the single-workgroup form of the push tail takes

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

} // namespace dppr
