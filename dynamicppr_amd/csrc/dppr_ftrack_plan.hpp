// dppr_ftrack_plan.hpp -- what a forward track (dppr_ftrack_*) decides before any device is involved: the limit on the tracks, the
// outputs of a call seen as those of dppr_forward_push, which epochs an update accepts, where the candidates of the first round come
// from, the sizes of the fix-up's scratch, and a plain host restatement of the fix-up (steps T and H) and of one SIGNED round over a
// small CSR. Pure host code without HIP includes (dppr_host_query.hpp checks a call and lays it out with it, dppr_ftrack.hpp takes
// its constants; tests/native/ftrack_plan_test.cpp drives it on the CPU under the sanitizers). The rounds, their lists and the row
// sum are those of dppr_fpush_plan.hpp / dppr_forward_plan.hpp.
//
// A CALL on the device (create: 1, 4, 5; update to the next epoch: all; update on the own epoch: 1, 4, 5; read: 1):
//     1 load     ext planes p | r  ->  the planes of the forward family by internal id, through the id map (every vertex with an id)
//     2 step T   the records sorted by tail (stable): a thread per (tail run, column) -> p, r of the tail, c per record of the run
//     3 step H   the records sorted by head (stable): a thread per (head run, column) walks its records in batch order -> r
//     4 rounds   dppr_fpush.hpp with the signed test; candidates of round 1: the records' tails and heads (a track that was
//                converged before the fix-up), else one scan of the live rows
//     5 store    back to the ext planes; |r| by internal id for the fold of rem
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "dppr_fpush_plan.hpp"

namespace dppr {

constexpr int FT_MAX = 16; // tracks of an engine (DPPR_FTRACK_MAX)
static_assert(DPPR_FTRACK_MAX == FT_MAX, "the limit of include/dppr.h");
static_assert(offsetof(dppr_ftrack_out_t, dense_layout) == offsetof(dppr_forward_push_out_t, dense_layout) &&
                  offsetof(dppr_ftrack_out_t, fix) == sizeof(dppr_forward_push_out_t) &&
                  offsetof(dppr_ftrack_out_t, work) == offsetof(dppr_forward_push_out_t, work) &&
                  offsetof(dppr_ftrack_out_t, at_r) == offsetof(dppr_forward_push_out_t, at_r),
              "dppr_ftrack_out_t is dppr_forward_push_out_t with fix behind it");

// ---- the call ------------------------------------------------------------------------------------------------------------------
enum : uint32_t { FT_FIX = 1u << 8 }; // beside FP_META .. FP_DENSE

// the outputs of a track call as those of a forward push (the checks and the parts are fp_parts_ok / fp_which)
inline dppr_forward_push_out_t ft_as_push(const dppr_ftrack_out_t &o) {
    dppr_forward_push_out_t q{};
    q.rounds_used = o.rounds_used; q.converged = o.converged; q.rem = o.rem; q.pushes = o.pushes; q.left = o.left;
    q.work = o.work;
    q.k = o.k; q.min_p = o.min_p; q.topk_ids = o.topk_ids; q.topk_p = o.topk_p; q.topk_counts = o.topk_counts;
    q.at_ids = o.at_ids; q.n_at = o.n_at; q.at_p = o.at_p; q.at_r = o.at_r;
    q.dense_p_dev = o.dense_p_dev; q.dense_r_dev = o.dense_r_dev; q.dense_dtype = o.dense_dtype; q.dense_layout = o.dense_layout;
    return q;
}
inline uint32_t ft_which(const dppr_ftrack_out_t *o) {
    if (!o) return 0;
    const dppr_forward_push_out_t q = ft_as_push(*o);
    return fp_which(&q) | (o->fix ? FT_FIX : 0u);
}
inline bool ft_parts_ok(const dppr_ftrack_out_t *o) {
    if (!o) return true; // (create and update may run without outputs)
    const dppr_forward_push_out_t q = ft_as_push(*o);
    return fp_parts_ok(&q);
}
// eps and max_rounds as dppr_forward_push takes them (out may be NULL here)
inline bool ft_create_args_ok(int32_t m, double eps, int32_t max_rounds) {
    dppr_forward_push_out_t q{};
    return fp_args_ok(m, eps, max_rounds, &q);
}
inline bool ft_rounds_ok(int32_t max_rounds) { return max_rounds >= 1 && max_rounds <= FP_MAX_ROUNDS; }
inline bool ft_handle_ok(int32_t track) { return track >= 0 && track < FT_MAX; }

// ---- the epochs an update accepts ------------------------------------------------------------------------------------------------
enum FtStep { FT_STEP_BAD = 0, FT_STEP_SAME = 1, FT_STEP_NEXT = 2 };
// `asked` is the resolved epoch number (never -1 here)
constexpr FtStep ft_step(int track_epoch, int asked) {
    return asked == track_epoch ? FT_STEP_SAME : asked == track_epoch + 1 ? FT_STEP_NEXT : FT_STEP_BAD;
}
// where the candidates of round 1 come from: the records (a fix-up on a track whose every column was converged) or one scan
constexpr bool ft_candidates_from_records(FtStep s, bool converged_before) { return s == FT_STEP_NEXT && converged_before; }

// ---- sizes -----------------------------------------------------------------------------------------------------------------------
// the ext planes of a track: p | r, each [V][row width]
constexpr size_t ft_state_elems(int64_t V, int gw) { return 2 * (size_t)(V > 0 ? V : 1) * (size_t)gw; }
// the fix-up's scratch for L records: keys in, keys out (by tail, by head), values in, values out (by tail, by head): 6 L words
constexpr size_t ft_sort_words(int L) { return 6 * (size_t)(L > 0 ? L : 1); }
// c per (record, column)
constexpr size_t ft_c_elems(int L, int gw) { return (size_t)(L > 0 ? L : 1) * (size_t)gw; }

// ---- the fix-up on the host ----------------------------------------------------------------------------------------------------------
// One column by vertex id: d1 [V] the stored out-degrees of the epoch the batch made, the L records in batch order. fix [3]:
// records applied, distinct tails, distinct heads.
inline void ft_fixup_ref(int V, double *p, double *r, const int *d1, int L, const int *tail, const int *head, const unsigned char *ins,
                         long long *fix) {
    std::vector<int> n_ins((size_t)V, 0), n_del((size_t)V, 0), is_head((size_t)V, 0);
    std::vector<double> c((size_t)V, 0.0);
    for (int i = 0; i < L; ++i) (ins[i] ? n_ins : n_del)[(size_t)tail[i]]++;
    long long tails = 0, heads = 0;
    for (int u = 0; u < V; ++u) { // step T
        if (!n_ins[(size_t)u] && !n_del[(size_t)u]) continue;
        ++tails;
        const int dd1 = d1[u], d0 = dd1 - n_ins[(size_t)u] + n_del[(size_t)u];
        const double den0 = (double)(d0 + 1);
        volatile double a = FW_ALPHA * den0;
        volatile double g = p[u] / a;
        volatile double cu = FW_DAMP * g;
        c[(size_t)u] = cu;
        if (dd1 != d0) {
            volatile double s = p[u] * (double)(dd1 + 1);
            volatile double q = s / den0;
            p[u] = q;
            volatile double t = (double)(dd1 - d0) * g;
            volatile double x = r[u] - t;
            r[u] = x;
        }
    }
    for (int i = 0; i < L; ++i) { // step H: per head in batch order == batch order
        const int w = head[i];
        if (!is_head[(size_t)w]) {
            is_head[(size_t)w] = 1;
            ++heads;
        }
        volatile double x = ins[i] ? r[w] + c[(size_t)tail[i]] : r[w] - c[(size_t)tail[i]];
        r[w] = x;
    }
    if (fix) {
        fix[0] = L;
        fix[1] = tails;
        fix[2] = heads;
    }
}

// ---- one signed round on the host ------------------------------------------------------------------------------------------------------
// fp_round_ref with F = { u : |r[u]| > thr[u] }. Returns |F|.
inline long long ft_round_ref(int V, const int *ptr, const int *tail, const int *d, double eps, double *p, double *r, double *y, int piece) {
    long long pushed = 0;
    for (int u = 0; u < V; ++u) {
        const double den = (double)(d[u] + 1);
        volatile double thr = eps * den;
        y[u] = 0.0;
        if (std::fabs(r[u]) > thr) {
            volatile double a = FW_ALPHA * r[u];
            p[u] = fw_add(p[u], a);
            volatile double b = FW_DAMP * r[u];
            volatile double q = b / den;
            y[u] = q;
            r[u] = 0.0;
            ++pushed;
        }
    }
    std::vector<double> t;
    for (int w = 0; w < V; ++w) {
        t.assign((size_t)(ptr[w + 1] - ptr[w]), 0.0);
        for (int e = ptr[w]; e < ptr[w + 1]; ++e) t[(size_t)(e - ptr[w])] = y[tail[e]];
        r[w] = fw_add(r[w], fw_row_sum_ref(t.data(), (long long)t.size(), piece));
    }
    return pushed;
}

} // namespace dppr
