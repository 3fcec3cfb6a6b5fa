// CPU test driver for dynamicppr_amd/csrc/dppr_loop_plan.hpp (the chunk and launch policy of the frontier loops and their
// histories). Every policy function against a plain restatement written here: the inline expression the loops held before the
// planner existed, transcribed, with the place it stood named (files and lines of commit 21acc1c, "Add, drop and replace sources
// of a running source group": H = dppr_host_loop.hpp, G = dppr_host_group.hpp). Small discrete inputs exhaustively, large ones
// seeded at random, and whole loops replayed through the planner's state struct and through the restatement's loose locals.
// One layer above the loops (commit 36757a9, "Move the frontier loops' chunk and launch policy into a tested planner": H2 =
// dppr_host_loop.hpp, E2 = dppr_engine.hip): what a whole-batch launch reported (ahead_outcome + apply_ahead against the tail of
// batch_ahead, H2:396-469) and what a batch runs after it (after_launch against dppr_update, E2:905-974), the latter driven by every
// outcome the former produces. And the state the single-source loop keeps between its launches (FrontierForm against the five loose
// flags of run_frontier_loop, commit dd4feff: H3 = dppr_host_loop.hpp): every sequence of up to six events the loop can enqueue.
//   loop_plan_test
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_loop_plan.hpp"

using namespace dppr;

static int fails = 0;
static long long checked = 0;
#define CHECK(c, ...) do { ++checked; if (!(c)) { if (fails++ < 10) { printf("FAILED %s (line %d): ", #c, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned long long rnd() { // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}
static long long rnd_below(long long n) { return (long long)(rnd() % (unsigned long long)n); }
// a value up to `top`, small ones as likely as large ones
static long long rnd_scaled(long long top) { return rnd_below((top >> rnd_below(32)) + 1); }

// ---------------------------------------------------------------------------- restatement: the values the kernels' headers fix
static const int R_MAX_CHUNK = 64, R_RESIDENT_MARGIN = 8, R_GMULTI_MAX = 128; // dppr_host_state.hpp:11, :22, :17
static const int R_RES_MAX_SWEEPS = 128;                                      // dppr_resident.hpp:99
static const int R_GPUSH_LOG = 16, R_TINY_N = 512, R_TINY_E = 1024;           // dppr_gpush.hpp:25, :264, :265

// ---------------------------------------------------------------------------- restatement: histories as loose arrays
struct RHist {
    int iter_hint[2], iter_hist[2][4], dense_hist[2][4]; // dppr_host_state.hpp:124-125 (Slot), :158-160 (Group)
};
static void r_record(RHist &h, int hp, int active_iters) { // H:347-349, H:477-479, G:379-381
    h.iter_hint[hp] = active_iters;
    for (int k = 3; k > 0; --k) h.iter_hist[hp][k] = h.iter_hist[hp][k - 1];
    h.iter_hist[hp][0] = active_iters;
}
static void r_record_dense(RHist &h, int hp, int v) { // G:376-377
    for (int k = 3; k > 0; --k) h.dense_hist[hp][k] = h.dense_hist[hp][k - 1];
    h.dense_hist[hp][0] = v;
}
static int r_lo(const int (&row)[4]) { // H:143-144, G:272-273
    int lo = 0;
    for (int h : row) lo = h > 0 && (lo == 0 || h < lo) ? h : lo;
    return lo;
}
static bool same(const LoopHistory &a, const RHist &b) {
    return !memcmp(a.hint, b.iter_hint, sizeof(a.hint)) && !memcmp(a.hist, b.iter_hist, sizeof(a.hist)) && !memcmp(a.dense, b.dense_hist, sizeof(a.dense));
}
static void fill(LoopHistory &a, RHist &b, int kind, int hp, int base) { // kind 0: all zero, 1: one entry, 2: full (both tables)
    a = LoopHistory();
    memset(&b, 0, sizeof(b));
    const int n = kind == 0 ? 0 : kind == 1 ? 1 : 4;
    for (int k = n - 1; k >= 0; --k) {
        const int v = base + (k * 7) % 5, d = std::max(1, v - 2 - k);
        a.record(hp, v); a.record_dense(hp, d);
        r_record(b, hp, v); r_record_dense(b, hp, d);
    }
}

// `follow *= 2` (G:285, H:148) overflows the int in a loop of more than thirty follow-up chunks, which is undefined (and stops this
// program): the planner stops doubling at 2^30, and so does the restatement -- the same value wherever the transcribed line has one
static void r_double(int &follow) {
    if (follow < (1 << 30)) follow *= 2;
}

// ---------------------------------------------------------------------------- restatement: source groups
static long long r_push_thr(int enter_pairs, int n_ggroups, int auto_factor) { // G:196
    return enter_pairs == 0 ? 0 : enter_pairs > 0 ? enter_pairs : std::max(64, n_ggroups * auto_factor);
}
static int r_multi(int iter_hint, int it, int chunk_iters, bool chunk_explicit) { // G:205-207
    int n = iter_hint > it ? iter_hint - it + R_RESIDENT_MARGIN : 2 * chunk_iters;
    n = std::max(2, std::min(n, R_GMULTI_MAX));
    if (chunk_explicit) n = std::min(n, std::max(chunk_iters, 2));
    return n;
}
static int r_group_chunk(const RHist &g, int hp, int it, long long liveF, long long push_thr, bool push_gave_up, int &follow, int chunk_iters,
                         bool chunk_explicit) { // G:270-288
    int n;
    if (it == 0) {
        int lo = 0;
        for (int h : (push_thr > 0 ? g.dense_hist : g.iter_hist)[hp]) lo = h > 0 && (lo == 0 || h < lo) ? h : lo;
        n = lo > 0 ? lo : chunk_iters;
        follow = 4;
    } else if (push_thr > 0 && !push_gave_up) {
        long long F = liveF; // (G:279-280: the sum of the live row)
        n = 1;
        for (long long f = F / 4; f > push_thr && n < chunk_iters; f /= 4) ++n;
    } else {
        n = std::min(follow, chunk_iters);
        r_double(follow);
    }
    if (chunk_explicit) n = std::min(n, std::max(chunk_iters, 1));
    n = std::max(1, std::min(n, R_MAX_CHUNK));
    return n;
}
static long long r_max_edges(long long gpush_max_edges, int n_ggroups) { // G:81
    return gpush_max_edges > 0 ? gpush_max_edges : std::max<long long>(4096, 20ll * std::max(n_ggroups, 1));
}
static int r_gpush_m(int it_done, long long pairs_at_entry) { // G:98-100
    int m = 2;
    if (it_done == 0)
        for (long long f = pairs_at_entry; f > 128 && m < R_GPUSH_LOG; f >>= 2) ++m;
    return m;
}

// ---------------------------------------------------------------------------- restatement: single source
static int r_pull_min(int setting, int Ed) { return setting > 0 ? setting : setting < 0 ? 0x7fffffff : std::max(1024, Ed / 192); } // H:39-41
static int r_single_chunk(bool trace, int chunk_iters, bool chunk_explicit, bool costly, bool pull, int F, int prevF, int pull_min, const RHist &s,
                          int hp, int it, bool can_reside, int &follow, bool *resident_out) { // H:124-152, :162
    int n;
    if (trace || chunk_iters <= 1) n = 1;
    else if (costly) n = (!pull && F < 4096 && F <= prevF) ? chunk_iters : 1;
    else if (pull) n = s.iter_hint[hp] > it ? s.iter_hint[hp] - it + 1 : chunk_iters;
    else if ((long long)F * 4 >= pull_min) n = 1;
    else n = F > prevF ? 2 : chunk_iters;
    const bool resident = pull && n >= 2 && !trace && can_reside; // (H:137: can_reside stands for the capacity and arena tests)
    if (resident && s.iter_hint[hp] > it) n += R_RESIDENT_MARGIN - 1;
    if (!resident && pull && n > 1) {
        int lo = 0;
        for (int h : s.iter_hist[hp]) lo = h > 0 && (lo == 0 || h < lo) ? h : lo;
        if (lo > it) n = lo - it;
        else if (lo > 0) {
            n = std::min(follow, chunk_iters);
            r_double(follow);
        }
    }
    n = std::min(n, R_MAX_CHUNK);
    if (chunk_explicit) n = std::min(n, std::max(chunk_iters, 1));
    if (resident) n = std::min(n, R_RES_MAX_SWEEPS); // H:162
    *resident_out = resident;
    return n;
}
static int r_batch_ahead(bool merged, const RHist &s, int chunk_iters, bool chunk_explicit) { // H:394-399
    int n = merged ? (s.iter_hint[0] > 0 ? std::min(s.iter_hint[0] + 2 * R_RESIDENT_MARGIN, 2 * R_MAX_CHUNK) : 2 * R_MAX_CHUNK)
            : s.iter_hint[0] > 0 && s.iter_hint[1] > 0
                      ? std::min(s.iter_hint[0] + s.iter_hint[1] + 1 + 2 * R_RESIDENT_MARGIN, 2 * R_MAX_CHUNK)
                      : 2 * R_MAX_CHUNK;
    if (chunk_explicit) n = std::min(n, chunk_iters);
    n = std::min(n, R_RES_MAX_SWEEPS);
    return n;
}

// ---------------------------------------------------------------------------- restatement: a whole batch of a single source
static const int R_CNT_HDR = 16;                                                           // dppr_host_state.hpp:14
static const int R_ABORTED = 1 << 30, R_FAULT = 1 << 29, R_CONVERGED = 1 << 28, R_PHASE1 = 1 << 26, R_SWEEPS = (1 << 16) - 1; // dppr_resident.hpp:127-131
static const int R_PHASE_BOTH = 2;                                                         // dppr_common.hpp:25
static const int R_RETRY_BATCHES = 64;                                                     // dppr_host_state.hpp:15
struct REntry { int it = 0; int F = -1; bool dense = false; bool any_pull = false; };      // H2:66-71
struct RSlot {                                                                             // what batch_ahead touches of Slot
    RHist hist;
    bool start_dense[2];
    int last_F0[2];
    long long iterations, pull_iterations, sum_F, persist_launches, persist_aborts;
};
struct REngine { bool launch_called_off; int raw_backoff; bool persist_ok; int persist_retry; }; // ... and of dppr_engine
// H2:396-469 (the profiling block, :418-423, reads HIP events and is left out). Returns 0, or 1 where the function fails.
static int r_ahead_tail(const int *pinned, int n, bool merged, bool inline_update, bool grouped, int pull_min, RSlot &s, REngine &e, int *stage,
                        REntry *en0, REntry *en1, bool *p1_seeded) {
    const int st = pinned[7];
    *stage = 0;
    *p1_seeded = false;
    *en0 = REntry();
    *en1 = REntry();
    s.persist_launches++;
    if (st & R_FAULT) return 1;
    e.launch_called_off = false;
    if ((st & R_ABORTED) && inline_update && !grouped && pinned[4] == 1) {
        e.launch_called_off = true;
        e.raw_backoff = 16;
        return 0;
    }
    if (st & R_ABORTED) {
        s.persist_aborts++;
        e.launch_called_off = true;
        e.persist_ok = false;
        e.persist_retry = R_RETRY_BATCHES;
        return 0;
    }
    const int pos = st & R_SWEEPS;
    int act[2] = {0, 0}, F0[2] = {0, 0}; // (H2:425: split_phase_log, as the loop it replaced -- H:452-468)
    long long log_sum = 0;
    for (int k = 0, ph = 0; k < std::min(pos + 1, n) && ph < 2; ++k) {
        if (pinned[R_CNT_HDR + k] <= 0) {
            ++ph;
            continue;
        }
        if (act[ph] == 0) F0[ph] = pinned[R_CNT_HDR + k];
        log_sum += pinned[R_CNT_HDR + k];
        act[ph]++;
    }
    for (int ph = 0; ph < 2; ++ph)
        if (act[ph] > 0) {
            s.start_dense[ph] = F0[ph] >= pull_min;
            s.last_F0[ph] = F0[ph];
        }
    s.iterations += act[0] + act[1];
    s.pull_iterations += act[0] + act[1];
    s.sum_F += log_sum;
    if (merged) {
        if (!(st & R_CONVERGED)) {
            en0->it = act[0];
            en0->F = pinned[0];
            en0->dense = true;
            en0->any_pull = true;
            return 0;
        }
        r_record(s.hist, 0, act[0]);
        if (act[0] == 0) s.start_dense[0] = false;
        *stage = 2;
        return 0;
    }
    if (!(st & R_PHASE1)) {
        en0->it = act[0];
        en0->F = pinned[0];
        en0->dense = true;
        en0->any_pull = true;
        return 0;
    }
    s.hist.iter_hint[0] = act[0];
    if (act[0] == 0) s.start_dense[0] = false;
    *stage = 1;
    *p1_seeded = true;
    if (!(st & R_CONVERGED)) {
        en1->it = act[1];
        en1->F = pinned[0];
        en1->dense = true;
        en1->any_pull = true;
        return 0;
    }
    s.hist.iter_hint[1] = act[1];
    if (act[1] == 0) s.start_dense[1] = false;
    *stage = 2;
    return 0;
}

// what a batch enqueues after its update, in order
enum { DO_REDO_UPDATE, DO_COUNT_RECORDS, DO_FILTER, DO_LOOP };
struct Did {
    int what, phase; // DO_LOOP: its phase
    bool flag;       // DO_FILTER: cnt[0..2] cleared first; DO_LOOP: seeded by a full Inspect (main_loop_inspect)
    REntry en;       // DO_LOOP without Inspect: the entry
};
static bool same(const REntry &a, const REntry &b) { return a.it == b.it && a.F == b.F && a.dense == b.dense && a.any_pull == b.any_pull; }
static bool same(const LoopEntry &a, const REntry &b) { return a.it == b.it && a.F == b.F && a.dense == b.dense && a.any_pull == b.any_pull; }
static bool same(const std::vector<Did> &a, const std::vector<Did> &b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); ++k)
        if (a[k].what != b[k].what || a[k].phase != b[k].phase || a[k].flag != b[k].flag || !same(a[k].en, b[k].en)) return false;
    return true;
}
// E2:905-974. The launch (made where `ahead`) reported called_off / stage / en0 / en1 / p1: what r_ahead_tail left.
static std::vector<Did> r_after_launch(bool merged, bool seeded, bool ahead, bool inline_su, bool called_off, int l_stage, REntry l_en0,
                                       REntry l_en1, bool l_p1) {
    std::vector<Did> did;
    auto stream_update = [&]() { did.push_back({DO_REDO_UPDATE, 0, false, REntry()}); };
    auto k_filter = [&](bool clear) { did.push_back({DO_FILTER, 0, clear, REntry()}); };
    auto run_frontier_loop = [&](int phase, REntry en = REntry()) { did.push_back({DO_LOOP, phase, false, en}); };
    auto main_loop_inspect = [&](int phase) { did.push_back({DO_LOOP, phase, true, REntry()}); };
    auto update_after_abort = [&]() {
        if (!inline_su) return;
        if (called_off) {
            inline_su = false;
            stream_update();
            return;
        }
        did.push_back({DO_COUNT_RECORDS, 0, false, REntry()});
    };
    if (merged && ahead) {
        int stage = l_stage;
        REntry en0 = l_en0;
        update_after_abort();
        if (stage != 2) {
            if (en0.it == 0 && !en0.dense) k_filter(false);
            run_frontier_loop(R_PHASE_BOTH, en0);
        }
    } else if (merged) {
        if (seeded) {
            k_filter(false);
            run_frontier_loop(R_PHASE_BOTH);
        } else {
            main_loop_inspect(R_PHASE_BOTH);
        }
    } else if (seeded) {
        int stage = 0;
        bool p1_seeded = false;
        REntry en0, en1;
        if (ahead) {
            stage = l_stage; en0 = l_en0; en1 = l_en1; p1_seeded = l_p1;
            update_after_abort();
        }
        if (stage == 0) run_frontier_loop(0, en0);
        if (stage <= 1 && !p1_seeded && inline_su) {
            main_loop_inspect(1);
        } else if (stage <= 1) {
            if (!p1_seeded) k_filter(true);
            run_frontier_loop(1, en1);
        }
    } else {
        main_loop_inspect(0);
        main_loop_inspect(1);
    }
    return did;
}
// ... and the same list from the planner's decision, executed as slot_update executes it
static std::vector<Did> planned_after_launch(const AfterLaunch &d) {
    std::vector<Did> did;
    if (d.redo_update) did.push_back({DO_REDO_UPDATE, 0, false, REntry()});
    if (d.count_records) did.push_back({DO_COUNT_RECORDS, 0, false, REntry()});
    for (int k = 0; k < d.n_loops; ++k) {
        const LoopStep &l = d.loop[k];
        if (d.filter && k == d.n_loops - 1) did.push_back({DO_FILTER, 0, d.filter_clears, REntry()});
        did.push_back({DO_LOOP, l.phase, l.inspect, l.inspect ? REntry() : REntry{l.entry.it, l.entry.F, l.entry.dense, l.entry.any_pull}});
    }
    return did;
}

// ---------------------------------------------------------------------------- restatement: which form of the frontier is live
// the five loose flags of run_frontier_loop and its assignments to them (commit dd4feff, "Host query layer: one state view and one
// call skeleton per family": H3 = dppr_host_loop.hpp), one event per place the loop enqueues something that changes them
struct RForm { bool extracted, dense_valid, list_valid, any_pull, x_clean; };
static RForm r_form(const REntry &en) { return {false, en.dense, !en.dense, en.any_pull, false}; } // H3:105-109
enum FormEvent { FE_LIST, FE_SNAP_RESIDENT, FE_RESIDENT_OPEN, FE_RESIDENT_CONVERGED, FE_SNAP, FE_SNAP_EXTRACT, FE_PUSH, FE_SWEEP, FE_COUNT };
static void r_apply(RForm &f, int ev) {
    switch (ev) {
    case FE_LIST: f.list_valid = true; break;            // H3:115 (make_list)
    case FE_SNAP_RESIDENT: f.dense_valid = true; break;  // H3:169 (the snapshot in front of a resident launch)
    case FE_RESIDENT_OPEN: case FE_RESIDENT_CONVERGED:   // H3:198-200
        f.list_valid = false; f.any_pull = true; f.x_clean = ev == FE_RESIDENT_CONVERGED; break;
    case FE_SNAP: case FE_SNAP_EXTRACT:                  // H3:214, :218 (the snapshot inside a chunk)
        f.extracted = ev == FE_SNAP_EXTRACT; f.dense_valid = true; break;
    case FE_PUSH: f.dense_valid = false; f.extracted = false; f.list_valid = true; break;                        // H3:286-288
    case FE_SWEEP: f.dense_valid = true; f.extracted = false; f.list_valid = false; f.any_pull = true; break;    // H3:235-238, :268-271
    }
}
static void p_apply(FrontierForm &f, int ev) {
    switch (ev) {
    case FE_LIST: f.list_made(); break;
    case FE_SNAP_RESIDENT: case FE_SNAP: f.snapshot_taken(false); break;
    case FE_SNAP_EXTRACT: f.snapshot_taken(true); break;
    case FE_RESIDENT_OPEN: f.resident_returned(false); break;
    case FE_RESIDENT_CONVERGED: f.resident_returned(true); break;
    case FE_PUSH: f.pushed(); break;
    case FE_SWEEP: f.swept(); break;
    }
}
// what the loop may enqueue next (its guards: H3:131, :147, :163 make a list only where none is valid; :166, :209 take a snapshot only
// where none is valid, from the list; a resident launch and a sweep read the snapshot, a push the list; the snapshot in front of a
// resident launch is followed by that launch, an extracting one by its push -- :214: extracted only where the iteration is no sweep;
// a converged launch ends the loop)
static bool may_follow(const RForm &f, int last, int ev) {
    if (last == FE_RESIDENT_CONVERGED) return false;
    if (last == FE_SNAP_RESIDENT) return ev == FE_RESIDENT_OPEN || ev == FE_RESIDENT_CONVERGED;
    if (last == FE_SNAP_EXTRACT) return ev == FE_PUSH;
    if (last == FE_SNAP) return ev == FE_PUSH || ev == FE_SWEEP;
    switch (ev) {
    case FE_LIST: return !f.list_valid;
    case FE_SNAP_RESIDENT: case FE_SNAP: case FE_SNAP_EXTRACT: return !f.dense_valid && f.list_valid;
    case FE_RESIDENT_OPEN: case FE_RESIDENT_CONVERGED: case FE_SWEEP: return f.dense_valid;
    default: return f.list_valid; // FE_PUSH (the eager schedule pushes without a snapshot)
    }
}
static long long form_sequences = 0;
static void walk_forms(const RForm &rf, const FrontierForm &pf, int last, int depth, bool entry_pull, bool swept) {
    // the planner's struct against the loose flags, and the combinations the loop relies on
    CHECK(pf.list == rf.list_valid && pf.dense == rf.dense_valid && pf.extracted == rf.extracted && pf.any_pull == rf.any_pull && pf.x_clean == rf.x_clean,
          "flags after event %d at depth %d", last, depth);
    CHECK(pf.needs_list() == !rf.list_valid && pf.needs_snapshot() == !rf.dense_valid && pf.must_zero_x() == (rf.any_pull && !rf.x_clean), "queries");
    CHECK(pf.list || pf.dense, "the frontier is live as a list, as a snapshot or as both: never as neither");
    CHECK(!pf.extracted || (pf.dense && last == FE_SNAP_EXTRACT), "an extracting snapshot lives until the push it was taken for, no longer");
    CHECK(last != FE_PUSH || (!pf.dense && pf.list), "after a push the snapshot is never valid, the list always");
    CHECK((last != FE_SWEEP && last != FE_RESIDENT_OPEN && last != FE_RESIDENT_CONVERGED) || (pf.dense && !pf.list && pf.any_pull), "a sweep leaves the snapshot alone");
    CHECK(pf.x_clean == (last == FE_RESIDENT_CONVERGED), "x is known clean only when a resident launch ended the loop");
    CHECK(pf.any_pull == (entry_pull || swept), "x is dirty once a sweep ran, here or in the launch before the entry");
    ++form_sequences;
    if (depth == 6) return;
    for (int ev = 0; ev < FE_COUNT; ++ev) {
        if (!may_follow(rf, last, ev)) continue;
        RForm r2 = rf;
        FrontierForm p2 = pf;
        r_apply(r2, ev);
        p_apply(p2, ev);
        walk_forms(r2, p2, ev, depth + 1, entry_pull, swept || ev == FE_SWEEP || ev == FE_RESIDENT_OPEN || ev == FE_RESIDENT_CONVERGED);
    }
}

// ---------------------------------------------------------------------------- whole loops of a group
// A loop is a sequence of frontier sizes (pairs): seq[i] is what sweep i finds, 0 beyond the end. What the push tail does
// when it is entered is scripted: it converges, or gives up once (after two iterations, handing back what the sequence
// holds there), or does not take the frontier once (it did not fit the lists).
enum TailScript { TAIL_CONVERGES, TAIL_GIVES_UP_ONCE, TAIL_OVERFLOWS_ONCE };
struct Step { int n; long long thr; int it; }; // a chunk as launched: its size, the threshold and the position it was sized at
static long long at(const std::vector<long long> &seq, int i) { return i < (int)seq.size() ? seq[(size_t)i] : 0; }
static int left(const std::vector<long long> &seq, int i) { return std::max(0, (int)seq.size() - i); }

static std::vector<Step> replay_restated(RHist &g, int hp, const std::vector<long long> &seq, int enter_pairs, int n_ggroups, int factor,
                                         int chunk_iters, bool chunk_explicit, bool multi, TailScript script) {
    std::vector<Step> out;
    bool more = at(seq, 0) > 0; // G:183
    int active_iters = 0;
    int follow = 4;             // G:191
    long long push_thr = r_push_thr(enter_pairs, n_ggroups, factor);
    bool push_gave_up = false;  // G:197
    int dense_len = -1;         // G:198
    bool scripted = false;
    for (int it = 0; more;) {
        if (multi) { // G:204-264
            const int n = r_multi(g.iter_hint[hp], it, chunk_iters, chunk_explicit);
            out.push_back({n, push_thr, it});
            const int sweeps = std::min(n, left(seq, it));
            for (int k = 0; k < sweeps; ++k) active_iters = it + k + 1;
            it += sweeps;
            more = at(seq, it) > 0;
            continue;
        }
        const int n = r_group_chunk(g, hp, it, at(seq, it), push_thr, push_gave_up, follow, chunk_iters, chunk_explicit);
        out.push_back({n, push_thr, it});
        for (int k = 0; k < n; ++k) { // G:317-344
            const long long F = at(seq, it + k);
            if (F <= 0) continue;
            if (push_thr > 0 && dense_len < 0) {
                if (F <= push_thr) dense_len = it + k;
            }
            active_iters = it + k + 1;
        }
        more = at(seq, it + n) > 0; // G:345-346
        it += n;
        if (more && push_thr > 0 && !push_gave_up) { // G:347-373
            const long long F = at(seq, it);
            if (F <= push_thr) {
                if (dense_len < 0) dense_len = it;
                const bool entered = !(script == TAIL_OVERFLOWS_ONCE && !scripted);
                const bool conv = script == TAIL_CONVERGES || scripted;
                const int pushed = !entered ? 0 : conv ? left(seq, it) : std::min(2, left(seq, it));
                scripted = true;
                if (entered) {
                    active_iters = it + pushed;
                    it += pushed;
                    if (conv) more = false;
                    else {
                        more = at(seq, it) > 0;
                        push_thr = std::max<long long>(F / 8, 1);
                        dense_len = -1;
                    }
                } else {
                    push_thr = std::max<long long>(F / 8, 1);
                    dense_len = -1;
                }
            }
        }
    }
    if (push_thr > 0) r_record_dense(g, hp, dense_len >= 0 ? std::max(dense_len, 1) : std::max(active_iters, 1)); // G:375-378
    r_record(g, hp, active_iters);                                                                                  // G:379-381
    return out;
}

static std::vector<Step> replay_planned(LoopHistory &g, int hp, const std::vector<long long> &seq, int enter_pairs, int n_ggroups, int factor,
                                        int chunk_iters, bool chunk_explicit, bool multi, TailScript script) {
    std::vector<Step> out;
    bool more = at(seq, 0) > 0;
    int active_iters = 0;
    GroupLoopPlan plan;
    plan.push_thr = group_push_threshold(enter_pairs, n_ggroups, factor);
    bool scripted = false;
    for (int it = 0; more;) {
        if (multi) {
            const int n = group_multi_sweeps(g.hint[hp], it, chunk_iters, chunk_explicit);
            out.push_back({n, plan.push_thr, it});
            const int sweeps = std::min(n, left(seq, it));
            if (sweeps > 0) active_iters = it + sweeps;
            it += sweeps;
            more = at(seq, it) > 0;
            continue;
        }
        const int n = plan.next_chunk(g, hp, it, at(seq, it), chunk_iters, chunk_explicit);
        out.push_back({n, plan.push_thr, it});
        for (int k = 0; k < n; ++k) {
            const long long F = at(seq, it + k);
            if (F <= 0) continue;
            plan.saw_frontier(F, it + k);
            active_iters = it + k + 1;
        }
        const long long F = at(seq, it + n);
        more = F > 0;
        it += n;
        if (plan.enter_push(more, F)) {
            plan.saw_frontier(F, it);
            const bool entered = !(script == TAIL_OVERFLOWS_ONCE && !scripted);
            const bool conv = script == TAIL_CONVERGES || scripted;
            const int pushed = !entered ? 0 : conv ? left(seq, it) : std::min(2, left(seq, it));
            scripted = true;
            if (entered) {
                active_iters = it + pushed;
                it += pushed;
                if (conv) more = false;
                else {
                    more = at(seq, it) > 0;
                    plan.push_declined(F);
                }
            } else {
                plan.push_declined(F);
            }
        }
    }
    plan.finish(g, hp, active_iters);
    return out;
}

static std::vector<long long> decay(long long f0, int num, int den, int plateau_at, int plateau_len) {
    std::vector<long long> seq;
    for (long long f = f0; f > 0; f = f * num / den) {
        seq.push_back(f);
        if ((int)seq.size() == plateau_at)
            for (int k = 0; k < plateau_len; ++k) seq.push_back(f);
        if (seq.size() > 400) break;
    }
    return seq;
}

int main() {
    static const int CHUNKS[] = {1, 2, 3, 24, 64};
    // ---- the restated constants
    CHECK(MAX_CHUNK == R_MAX_CHUNK && RESIDENT_MARGIN == R_RESIDENT_MARGIN && GMULTI_MAX == R_GMULTI_MAX, "host constants");
    CHECK(PLAN_RES_MAX_SWEEPS == R_RES_MAX_SWEEPS && PLAN_GPUSH_LOG == R_GPUSH_LOG && PLAN_TINY_N == R_TINY_N && PLAN_TINY_E == R_TINY_E, "kernel constants");

    // ---- histories: record / shortest against the shift loops and the scans; save and restore around a loop (group_solve_column)
    {
        LoopHistory a;
        RHist b;
        memset(&b, 0, sizeof(b));
        CHECK(same(a, b), "a fresh history is all zero");
        for (int i = 0; i < 200; ++i) {
            const int hp = (int)rnd_below(2), v = (int)rnd_below(90);
            if (rnd_below(3)) { a.record(hp, v); r_record(b, hp, v); }
            else { a.record_dense(hp, v); r_record_dense(b, hp, v); }
            CHECK(same(a, b), "history after %d records", i + 1);
            for (int p = 0; p < 2; ++p) {
                CHECK(a.shortest(p) == r_lo(b.iter_hist[p]), "shortest(%d)", p);
                CHECK(a.shortest_dense(p) == r_lo(b.dense_hist[p]), "shortest_dense(%d)", p);
            }
            // G:391-398: the three arrays saved with memcpy, a loop run, the arrays put back
            int hint[2], hist[2][4], dense[2][4];
            memcpy(hint, b.iter_hint, sizeof(hint)); memcpy(hist, b.iter_hist, sizeof(hist)); memcpy(dense, b.dense_hist, sizeof(dense));
            const LoopHistory kept = a, before = a;
            a.record(0, 1 + (int)rnd_below(50)); a.record_dense(0, 1 + (int)rnd_below(50));
            r_record(b, 0, 77); r_record_dense(b, 0, 5);
            a = kept;
            memcpy(b.iter_hint, hint, sizeof(hint)); memcpy(b.iter_hist, hist, sizeof(hist)); memcpy(b.dense_hist, dense, sizeof(dense));
            CHECK(!memcmp(&a, &before, sizeof(a)) && same(a, b), "save / restore around a from-scratch loop");
        }
    }

    // ---- every combination of the small inputs
    for (int it = 0; it <= 70; ++it)
        for (int chunk_iters : CHUNKS)
            for (int expl = 0; expl < 2; ++expl)
                for (int kind = 0; kind < 3; ++kind)
                    for (int hp = 0; hp < 2; ++hp)
                        for (int base : {1, 5, 30, 69}) {
                            LoopHistory a;
                            RHist b;
                            fill(a, b, kind, hp, base);
                            CHECK(group_multi_sweeps(a.hint[hp], it, chunk_iters, expl) == r_multi(b.iter_hint[hp], it, chunk_iters, expl), "multi it %d", it);
                            for (int merged = 0; merged < 2; ++merged)
                                CHECK(batch_ahead_sweeps(merged, a, chunk_iters, expl) == r_batch_ahead(merged, b, chunk_iters, expl), "batch_ahead");
                            // the group's one-sweep chunks: no push form, push form armed (frontier far above, near and below the threshold), given up
                            for (long long thr : {0ll, 64ll, 6150ll})
                                for (int gave_up = 0; gave_up < 2; ++gave_up)
                                    for (long long F : {1ll, 63ll, 300ll, 30000ll, 5000000ll})
                                        for (int follow0 : {4, 8, 64}) {
                                            GroupLoopPlan plan;
                                            plan.push_thr = thr; plan.push_gave_up = gave_up; plan.follow = follow0;
                                            int follow = follow0;
                                            const int want = r_group_chunk(b, hp, it, F, thr, gave_up, follow, chunk_iters, expl);
                                            const int got = plan.next_chunk(a, hp, it, F, chunk_iters, expl);
                                            CHECK(got == want && plan.follow == follow, "group chunk it %d chunk %d expl %d kind %d thr %lld F %lld: %d / %d, follow %d / %d",
                                                  it, chunk_iters, expl, kind, thr, F, got, want, plan.follow, follow);
                                        }
                            // the single-source chunk
                            for (int flags = 0; flags < 16; ++flags) {
                                const bool trace = flags & 1, costly = flags & 2, pull = flags & 4, can_reside = flags & 8;
                                for (int F : {1, 300, 4095, 4096, 100000})
                                    for (int prevF : {0, 300, 200000})
                                        for (int pull_min : {1, 1024, 0x7fffffff}) {
                                            int follow_r = 4, follow_p = 4;
                                            bool res_r = false;
                                            const int want = r_single_chunk(trace, chunk_iters, expl, costly, pull, F, prevF, pull_min, b, hp, it, can_reside, follow_r, &res_r);
                                            int n = single_chunk(trace, chunk_iters, costly, pull, F, prevF, pull_min, a.hint[hp], it);
                                            const bool res_p = pull && n >= 2 && !trace && can_reside;
                                            n = single_chunk_for_form(n, res_p, pull, a, hp, it, follow_p, chunk_iters, expl);
                                            CHECK(n == want && res_p == res_r && follow_p == follow_r, "single chunk it %d chunk %d flags %d F %d prevF %d: %d / %d", it,
                                                  chunk_iters, flags, F, prevF, n, want);
                                        }
                            }
                        }

    // ---- seeded random large inputs
    for (int i = 0; i < 400000; ++i) {
        const long long F = rnd_scaled(1ll << 31), thr = rnd_scaled(1ll << 31);
        const int n_ggroups = (int)rnd_scaled(1 << 20), factor = 1 + (int)rnd_below(64), enter = (int)rnd_scaled(0x7fffffff) - (int)rnd_below(2);
        const int chunk_iters = CHUNKS[rnd_below(5)], it = (int)rnd_below(71), hp = (int)rnd_below(2);
        const bool expl = rnd_below(2), gave_up = rnd_below(8) == 0;
        CHECK(group_push_threshold(enter, n_ggroups, factor) == r_push_thr(enter, n_ggroups, factor), "threshold %d %d %d", enter, n_ggroups, factor);
        CHECK(group_push_threshold(-1, n_ggroups, factor) == r_push_thr(-1, n_ggroups, factor), "automatic threshold %d %d", n_ggroups, factor);
        const long long cfg = rnd_below(4) ? 0 : rnd_scaled(1ll << 40);
        CHECK(gpush_edge_bound(cfg, n_ggroups) == r_max_edges(cfg, n_ggroups), "edge bound %lld %d", cfg, n_ggroups);
        const int it_done = (int)rnd_below(3);
        CHECK(gpush_chunk(it_done, F) == r_gpush_m(it_done, F), "push chunk %d %lld", it_done, F);
        CHECK(gpush_adds_at_entry(F) == (F <= 64 ? 0 : -1), "adds at entry %lld", F); // G:87
        const long long known_n = rnd_scaled(1 << 12), adds = rnd_scaled(1 << 12) - 1;
        const bool declined = rnd_below(2), stop = rnd_below(2), progressed = rnd_below(2);
        CHECK(gpush_take_tiny(known_n, adds, declined) == (known_n <= R_TINY_N && adds >= 0 && adds <= R_TINY_E / 2 && !declined), "tiny form"); // G:89
        CHECK(gpush_tiny_declined(progressed, stop, known_n) == (!progressed && !stop && known_n <= R_TINY_N), "tiny declined");               // G:126
        LoopHistory a;
        RHist b;
        fill(a, b, (int)rnd_below(3), hp, 1 + (int)rnd_below(69));
        GroupLoopPlan plan;
        plan.push_thr = thr; plan.push_gave_up = gave_up; plan.follow = 4 << rnd_below(10);
        int follow = plan.follow;
        const int want = r_group_chunk(b, hp, it, F, thr, gave_up, follow, chunk_iters, expl);
        CHECK(plan.next_chunk(a, hp, it, F, chunk_iters, expl) == want && plan.follow == follow, "group chunk F %lld thr %lld", F, thr);
        CHECK(plan.enter_push(F > 0, F) == (F > 0 && thr > 0 && !gave_up && F <= thr), "enter push F %lld thr %lld", F, thr); // G:347-350
        plan.push_declined(F);
        CHECK(plan.push_thr == std::max<long long>(F / 8, 1) && plan.dense_len == -1, "back-off F %lld", F); // G:365-366, :369-370
        // single source
        const int setting = (int)rnd_below(3) - 1 ? (int)rnd_scaled(0x7fffffff) : -(int)rnd_below(2), Ed = (int)rnd_scaled(0x7fffffff);
        CHECK(pull_min_frontier(setting, Ed) == r_pull_min(setting, Ed), "pull_min %d %d", setting, Ed);
        const double mean = rnd_below(3) ? (double)rnd_scaled(1 << 20) / 7.0 : 0.0, atomic_ns = 0.02 + (double)rnd_below(1000) / 1000.0;
        const bool binned = rnd_below(2);
        const int Fi = (int)rnd_scaled(0x7fffffff);
        const long long D = rnd_below(4) ? rnd_scaled(1ll << 36) : -1;
        CHECK(window_costly(binned, expl, mean, Ed) == (binned && !expl && (mean > 0 ? mean : 6.5e-6 * (double)Ed) >= 300.0), "costly"); // H:100
        CHECK(cost_needs_degrees(Fi, D) == (D < 0 && Fi >= 1024), "degrees wanted");                                                  // H:107
        CHECK(cost_decides(Fi, D) == (D >= 0 || Fi < 1024), "cost decides");                                                         // H:118
        {
            const double sweep_us = mean > 0 ? mean : 6.5e-6 * (double)Ed;                               // H:119
            const double push_us = 15.0 + (double)std::max<long long>(D, 0) * atomic_ns * 1e-3;          // H:120
            CHECK(cost_says_sweep(Fi, D, mean, Ed, atomic_ns) == (Fi >= 1024 && push_us > 0.9 * sweep_us), "push or sweep"); // H:121
        }
        const float ms = (float)rnd_scaled(1 << 20) / 1024.0f;
        const double want_sweep = mean > 0 ? 0.75 * mean + 0.25 * ms * 1e3 : ms * 1e3; // H:333
        CHECK(mean_sweep_us(mean, ms) == want_sweep, "mean of the sweeps");
        const double want_atomic = D >= (1 << 20) ? 0.75 * atomic_ns + 0.25 * std::min(1.0, std::max(0.02, (ms * 1e6 - 15e3) / (double)D)) : atomic_ns; // H:334
        CHECK(mean_atomic_ns(atomic_ns, ms, D) == want_atomic, "mean of the atomics");
    }

    // ---- the log of a whole-batch launch (H:452-468)
    for (int i = 0; i < 20000; ++i) {
        int log[40];
        const int entries = (int)rnd_below(41);
        for (int &v : log) v = rnd_below(4) ? (int)rnd_scaled(1 << 30) : 0;
        const int pull_min = (int)rnd_scaled(1 << 30);
        long long iterations = 0, sum_F = 0;
        bool start_dense[2] = {false, true};
        int last_F0[2] = {-5, -6};
        int act[2] = {0, 0}, ph = 0;
        for (int k = 0; k < entries && ph < 2; ++k) {
            if (log[k] <= 0) {
                ++ph;
                continue;
            }
            if (act[ph] == 0) {
                start_dense[ph] = log[k] >= pull_min;
                last_F0[ph] = log[k];
            }
            iterations++;
            sum_F += log[k];
            act[ph]++;
        }
        const PhaseLog pl = split_phase_log(log, entries);
        CHECK(pl.act[0] == act[0] && pl.act[1] == act[1] && pl.sum_F == sum_F && pl.act[0] + pl.act[1] == iterations, "phase log counts");
        for (int p = 0; p < 2; ++p)
            if (act[p] > 0) CHECK(pl.F0[p] == last_F0[p] && (pl.F0[p] >= pull_min) == start_dense[p], "first frontier of phase %d", p);
    }

    // ---- whole loops, eight batches one after the other so that the histories feed the next loop's chunks
    {
        struct Shape { long long f0; int num, den, plateau_at, plateau_len; };
        const Shape shapes[] = {{4000000, 1, 3, 0, 0}, {4000000, 1, 3, 5, 6}, {900, 1, 2, 0, 0}, {123456789, 2, 5, 9, 3}, {2000000000, 1, 4, 0, 0}, {70, 9, 10, 3, 20}};
        long long steps = 0;
        for (const Shape &sh : shapes)
            for (int chunk_iters : CHUNKS)
                for (int expl = 0; expl < 2; ++expl)
                    for (int enter : {-1, 0, 50, 1000000000})
                        for (int multi = 0; multi < 2; ++multi)
                            for (int script = 0; script < 3; ++script) {
                                LoopHistory a;
                                RHist b;
                                memset(&b, 0, sizeof(b));
                                for (int batch = 0; batch < 8; ++batch) {
                                    // (consecutive batches take about the same number of sweeps, not exactly)
                                    std::vector<long long> seq = decay(sh.f0 + 977 * batch, sh.num, sh.den, sh.plateau_at, sh.plateau_len + batch % 3);
                                    const int hp = batch & 1 && !multi ? 1 : 0;
                                    const std::vector<Step> want = replay_restated(b, hp, seq, enter, 3075, 2, chunk_iters, expl, multi, (TailScript)script);
                                    const std::vector<Step> got = replay_planned(a, hp, seq, enter, 3075, 2, chunk_iters, expl, multi, (TailScript)script);
                                    CHECK(got.size() == want.size() && !got.empty(), "chunks of a loop: %zu / %zu", got.size(), want.size());
                                    for (size_t k = 0; k < std::min(got.size(), want.size()); ++k)
                                        CHECK(got[k].n == want[k].n && got[k].thr == want[k].thr && got[k].it == want[k].it,
                                              "chunk %zu: n %d / %d, threshold %lld / %lld, at %d / %d", k, got[k].n, want[k].n, got[k].thr, want[k].thr, got[k].it, want[k].it);
                                    CHECK(same(a, b), "histories after batch %d", batch);
                                    steps += (long long)got.size();
                                }
                            }
        CHECK(steps > 10000, "the replays launched %lld chunks", steps);
        // the scripts did what they are named for: a give-up and an overflow each lower the threshold mid-loop
        for (int script = 1; script < 3; ++script) {
            LoopHistory a;
            const std::vector<Step> st = replay_planned(a, 0, decay(4000000, 1, 3, 0, 0), -1, 3075, 2, 2, false, false, (TailScript)script);
            bool lowered = false;
            for (size_t k = 1; k < st.size(); ++k) lowered |= st[k].thr < st[k - 1].thr;
            CHECK(lowered, "script %d never lowered the threshold", script);
        }
    }
    // ---- a whole-batch launch: its outcome, what it leaves in the slot, and what the batch runs after it
    {
        CHECK(PERSIST_ABORTED == R_ABORTED && PERSIST_FAULT == R_FAULT && PERSIST_CONVERGED == R_CONVERGED && PERSIST_PHASE1 == R_PHASE1 &&
                  PERSIST_SWEEPS == R_SWEEPS && LOOP_PHASE_BOTH == R_PHASE_BOTH, "status bits");
        bool reached[2][2][4][3][2][2][2] = {}; // merged, inline_update, kind, stage, p1_seeded, entry.it == 0, entry.dense
        long long outcomes = 0;
        for (int n : {1, 2, 3, 5, 64, 128}) {
            // the logs: no zero at all; a zero in one position, every position in turn (0: a leading zero); two adjacent zeros,
            // every position in turn; random ones with a zero in every fourth place or so
            std::vector<std::vector<int>> logs;
            auto fresh = [&]() {
                std::vector<int> l((size_t)n);
                for (int &v : l) v = 1 + (int)rnd_scaled(1 << 30);
                return l;
            };
            logs.push_back(fresh());
            for (int z = 0; z < n; ++z) {
                logs.push_back(fresh());
                logs.back()[(size_t)z] = 0;
                if (z + 1 < n) {
                    logs.push_back(fresh());
                    logs.back()[(size_t)z] = logs.back()[(size_t)z + 1] = 0;
                }
            }
            for (int k = 0; k < 24; ++k) {
                logs.push_back(fresh());
                for (int &v : logs.back())
                    if (!rnd_below(4)) v = 0;
            }
            for (const std::vector<int> &log : logs)
                for (int bits = 0; bits < 16; ++bits)
                    for (int pos : {0, 1, 2, n - 1, n, n + 1})
                        for (int cnt4 = 0; cnt4 < 2; ++cnt4)
                            for (int flags = 0; flags < 8; ++flags) {
                                const bool merged = flags & 1, inline_update = flags & 2, grouped = flags & 4;
                                const int status = pos | (bits & 1 ? R_ABORTED : 0) | (bits & 2 ? R_FAULT : 0) | (bits & 4 ? R_CONVERGED : 0) | (bits & 8 ? R_PHASE1 : 0);
                                int pinned[R_CNT_HDR + 128];
                                for (int k = 0; k < R_CNT_HDR; ++k) pinned[k] = (int)rnd_scaled(1 << 30);
                                pinned[7] = status;
                                pinned[4] = cnt4;
                                memcpy(pinned + R_CNT_HDR, log.data(), sizeof(int) * (size_t)n);
                                const int pull_min = rnd_below(3) ? (int)rnd_scaled(1 << 30) : 0x7fffffff;
                                // the slot as some earlier batches left it, the same on both sides
                                LoopHistory hist;
                                RSlot rs;
                                fill(hist, rs.hist, (int)rnd_below(3), (int)rnd_below(2), 1 + (int)rnd_below(69));
                                bool start_dense[2];
                                int last_F0[2];
                                for (int ph = 0; ph < 2; ++ph) {
                                    start_dense[ph] = rs.start_dense[ph] = rnd_below(2);
                                    last_F0[ph] = rs.last_F0[ph] = (int)rnd_scaled(1 << 30);
                                }
                                int64_t iterations = rnd_scaled(1ll << 40), pull_iterations = rnd_scaled(1ll << 40), sum_F = rnd_scaled(1ll << 50);
                                const int64_t iterations0 = iterations, sum_F0 = sum_F;
                                rs.iterations = iterations; rs.pull_iterations = pull_iterations; rs.sum_F = sum_F;
                                rs.persist_launches = rs.persist_aborts = 0;
                                REngine re{false, 0, true, 0};
                                int stage = -1;
                                bool p1 = true;
                                REntry en0, en1;
                                const int rc = r_ahead_tail(pinned, n, merged, inline_update, grouped, pull_min, rs, re, &stage, &en0, &en1, &p1);

                                const AheadOutcome o = ahead_outcome(pinned[7], pinned[4], pinned[0], pinned + R_CNT_HDR, n, merged, inline_update, grouped);
                                apply_ahead(o, merged, pull_min, hist, start_dense, last_F0, iterations, pull_iterations, sum_F);
                                ++outcomes;
                                // the kind against the four ways out of the transcription
                                const AheadKind want = rc ? AHEAD_FAULT : !re.launch_called_off ? AHEAD_RAN : rs.persist_aborts ? AHEAD_CALLED_OFF_ROLLCALL : AHEAD_CALLED_OFF_RECORDS;
                                CHECK(o.kind == want, "kind %d / %d (status 0x%x cnt4 %d flags %d)", (int)o.kind, (int)want, (unsigned)status, cnt4, flags);
                                CHECK(o.called_off() == (!rc && re.launch_called_off), "called off");
                                CHECK((o.kind == AHEAD_CALLED_OFF_RECORDS) == (re.raw_backoff == 16) && (o.kind == AHEAD_CALLED_OFF_ROLLCALL) == (!re.persist_ok && re.persist_retry == R_RETRY_BATCHES),
                                      "a records call-off backs the raw records off and counts no abort; a failed roll-call counts one and re-arms later");
                                CHECK(o.stage == stage && o.p1_seeded == p1, "stage %d / %d, p1_seeded %d / %d (status 0x%x n %d flags %d)", o.stage, stage, (int)o.p1_seeded, (int)p1,
                                      (unsigned)status, n, flags);
                                // the one entry to resume with is that of the open loop; the transcription's other one is as constructed
                                CHECK(same(o.entry, stage == 1 ? en1 : en0) && same(stage == 1 ? en0 : en1, REntry()) && (stage < 2 || same(en0, REntry())),
                                      "entry it %d F %d (stage %d status 0x%x n %d flags %d)", o.entry.it, o.entry.F, stage, (unsigned)status, n, flags);
                                CHECK(same(hist, rs.hist), "histories (status 0x%x n %d flags %d)", (unsigned)status, n, flags);
                                CHECK(!memcmp(start_dense, rs.start_dense, sizeof(start_dense)) && !memcmp(last_F0, rs.last_F0, sizeof(last_F0)), "start_dense / last_F0");
                                CHECK(iterations == rs.iterations && pull_iterations == rs.pull_iterations && sum_F == rs.sum_F, "iterations / pull_iterations / sum_F");
                                // the log it carries is the one it was applied from; a launch that did not run carries none
                                CHECK(iterations - iterations0 == o.log.act[0] + o.log.act[1] && sum_F - sum_F0 == o.log.sum_F && (o.kind == AHEAD_RAN || o.log.act[0] + o.log.act[1] == 0), "log");
                                reached[merged][inline_update][o.kind][o.stage][o.p1_seeded][o.entry.it == 0][o.entry.dense] = true;
                                if (rc) continue; // (dppr_update returned the error)
                                // what the batch runs after this launch: a launch is made from a converged state only (ahead => seeded),
                                // and only a launch applies the records itself (inline_su => ahead)
                                const std::vector<Did> want_did = r_after_launch(merged, true, true, inline_update, re.launch_called_off, stage, en0, en1, p1);
                                const std::vector<Did> got_did = planned_after_launch(after_launch(merged, true, true, inline_update, o));
                                CHECK(same(got_did, want_did) && !want_did.empty() == (stage != 2 || inline_update), "after the launch: %zu / %zu steps (status 0x%x n %d flags %d)",
                                      got_did.size(), want_did.size(), (unsigned)status, n, flags);
                            }
        }
        CHECK(outcomes > 500000, "%lld outcomes", outcomes);
        // ... and without a launch
        for (int flags = 0; flags < 4; ++flags) {
            const bool merged = flags & 1, seeded = flags & 2;
            const std::vector<Did> want_did = r_after_launch(merged, seeded, false, false, false, 0, REntry(), REntry(), false);
            CHECK(same(planned_after_launch(after_launch(merged, seeded, false, false, AheadOutcome())), want_did) && want_did.size() >= 1, "no launch, flags %d", flags);
        }
        // what the enumeration reached of merged x inline_update x kind x stage x p1_seeded x (entry.it == 0) x entry.dense: every kind
        // in every plan; a merged launch stops at stage 0 or 2 and seeds no phase 1; an entry is dense exactly where a launch ran out
        // of sweeps, and then may well be at position 0 (a launch that was given one sweep)
        int n_reached = 0;
        for (int m = 0; m < 2; ++m)
            for (int iu = 0; iu < 2; ++iu)
                for (int kind = 0; kind < 4; ++kind)
                    for (int stage = 0; stage < 3; ++stage)
                        for (int p1 = 0; p1 < 2; ++p1)
                            for (int it0 = 0; it0 < 2; ++it0)
                                for (int dense = 0; dense < 2; ++dense) {
                                    if (!reached[m][iu][kind][stage][p1][it0][dense]) continue;
                                    ++n_reached;
                                    CHECK(kind == AHEAD_RAN || (stage == 0 && !p1 && it0 && !dense), "a launch that did not run leaves stage 0 and no entry");
                                    CHECK(!m || (stage != 1 && !p1), "a merged launch has no phase 1");
                                    CHECK(m || p1 == (stage >= 1), "two phases: phase 1 is seeded by the launch that finished phase 0");
                                    CHECK(kind != AHEAD_RAN || dense == (stage < 2), "the entry of an open loop holds its snapshot");
                                    CHECK(kind != AHEAD_CALLED_OFF_RECORDS || iu, "only a launch that applies the records calls itself off over them");
                                }
        for (int m = 0; m < 2; ++m) {
            for (int iu = 0; iu < 2; ++iu) {
                CHECK(reached[m][iu][AHEAD_FAULT][0][0][1][0] && reached[m][iu][AHEAD_CALLED_OFF_ROLLCALL][0][0][1][0], "fault and failed roll-call, merged %d inline %d", m, iu);
                CHECK(reached[m][iu][AHEAD_RAN][0][0][0][1] && reached[m][iu][AHEAD_RAN][0][0][1][1] && reached[m][iu][AHEAD_RAN][2][!m][1][0], "out of sweeps / done, merged %d inline %d", m, iu);
            }
            CHECK(reached[m][1][AHEAD_CALLED_OFF_RECORDS][0][0][1][0], "records call-off, merged %d", m);
        }
        CHECK(reached[0][0][AHEAD_RAN][1][1][0][1] && reached[0][0][AHEAD_RAN][1][1][1][1], "phase 1 open");
        // fault and failed roll-call in each of the four plans, the records call-off in the two that apply them: 10; the merged loop
        // open at position 0 / further on, or done, in its two plans: 6; phase 0 open (twice), phase 1 open (twice), done, in two plans: 10
        CHECK(n_reached == 10 + 6 + 10, "%d combinations reached", n_reached);
        // the branch no GPU test drove before: the merged loop after a records call-off is the update's own kernels, the negative
        // tails added WITHOUT clearing the counters, and the loop over both signs from its start
        {
            const int log1[1] = {0};
            const AheadOutcome o = ahead_outcome(R_ABORTED, 1, 0, log1, 1, true, true, false);
            const AfterLaunch d = after_launch(true, true, true, true, o);
            CHECK(o.kind == AHEAD_CALLED_OFF_RECORDS && d.redo_update && !d.count_records && d.filter && !d.filter_clears && d.n_loops == 1 &&
                      d.loop[0].phase == LOOP_PHASE_BOTH && !d.loop[0].inspect && same(d.loop[0].entry, REntry()), "merged loop after a records call-off");
        }
    }
    // ---- which form of a single-source loop's frontier is live: every sequence of up to six events the loop can enqueue, from a loop's
    // start (the list) and from where a whole-batch launch ran out of sweeps (its snapshot)
    {
        const REntry starts[2] = {REntry(), REntry{5, 77, true, true}};
        for (const REntry &en : starts) {
            const long long before = form_sequences;
            walk_forms(r_form(en), FrontierForm(LoopEntry{en.it, en.F, en.dense, en.any_pull}), -1, 0, en.any_pull, false);
            CHECK(form_sequences - before > 500, "%lld event sequences from entry dense %d", form_sequences - before, (int)en.dense);
        }
    }
    printf("%lld checks, %d failures\n", checked, fails);
    return fails ? 1 : 0;
}
