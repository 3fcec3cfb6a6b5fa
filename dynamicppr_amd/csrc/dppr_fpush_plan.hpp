// dppr_fpush_plan.hpp -- what the forward push (dppr_forward_push) decides before any device is involved: the limits, the checks
// of the arguments and of the start sets' CSR, which parts of dppr_forward_push_out_t a call asks for, the schedule of the round
// chunks (rounds enqueued between two read-backs of ONE word), the sizes of the bitmap and of the lists, the grids, the work
// space, and a plain host restatement of one round over a small CSR. Pure host code without HIP includes (dppr_host_query.hpp
// checks a call and lays it out with it, dppr_fpush.hpp takes its constants; tests/native/fpush_plan_test.cpp drives it on the
// CPU under the sanitizers). The row sum, its pieces and their lists are those of dppr_forward_plan.hpp.
//
// A ROUND on the device, k = 1, 2, .. with b = k & 1 (the lists and the y planes alternate, so nothing is cleared while it is read):
//     select   over the candidates recv[b ^ 1]: r > thr per column; p, y[b], r; the rows with any column pushed enter front[b],
//              the pieces of their out-rows enter the mark list; y[b ^ 1] of front[b ^ 1] is cleared
//     mark     over the mark list: a bit per head; the first setter enters recv[b] (a long in-row also the lists of its pieces)
//     gather   over recv[b]: r += the row sum over y[b]; long rows through pieces (k_fw_pieces) and k_fp_long
// The candidates of round k + 1 are the receivers of round k and nothing else: a pushed vertex has r = +0.0 until it receives,
// and a vertex that failed the comparison fails it until it receives.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#include "dppr_forward_plan.hpp"
#include "dppr_targets_plan.hpp"

namespace dppr {

constexpr int FP_SET_MAX = 4096;     // seeds of a column (DPPR_FPUSH_SET_MAX)
constexpr int FP_MAX_ROUNDS = 256;   // DPPR_FPUSH_MAX_ROUNDS
constexpr int FP_CHUNK = 8;          // rounds enqueued between two read-backs (dppr_debug_forward_push changes it)
constexpr int FP_MARK_LANES = 16;    // lanes that walk one piece of an out-row
constexpr int FP_MARK_PIECE = 128;   // out-edges of such a piece: 8 trips of 16 lanes
constexpr int FP_GRID_MAX = 1024;    // every round kernel loops grid-stride over a count it reads from device memory
static_assert(DPPR_FPUSH_SET_MAX == FP_SET_MAX && DPPR_FPUSH_MAX_ROUNDS == FP_MAX_ROUNDS, "the limits of include/dppr.h");
static_assert(FP_MARK_PIECE % FP_MARK_LANES == 0 && 64 % FP_MARK_LANES == 0, "a wave walks whole pieces");

// ---- the call ------------------------------------------------------------------------------------------------------------------
enum : uint32_t { FP_META = 1u << 0, FP_WORK = 1u << 1, FP_TOPK = 1u << 2, FP_AT = 1u << 3, FP_DENSE = 1u << 4 };

inline uint32_t fp_which(const dppr_forward_push_out_t *o) {
    if (!o) return 0;
    uint32_t w = 0;
    if (o->rounds_used || o->converged || o->rem || o->pushes || o->left) w |= FP_META;
    if (o->work) w |= FP_WORK;
    if (o->topk_ids || o->topk_p || o->topk_counts) w |= FP_TOPK;
    if (o->at_ids || o->at_p || o->at_r) w |= FP_AT;
    if (o->dense_p_dev || o->dense_r_dev) w |= FP_DENSE;
    return w;
}
// eps > 0 is false for a NaN; an infinite eps is refused too
inline bool fp_args_ok(int32_t m, double eps, int32_t max_rounds, const dppr_forward_push_out_t *out) {
    return out && m >= 1 && m <= DPPR_FORWARD_MAX_M && eps > 0.0 && std::isfinite(eps) && max_rounds >= 1 && max_rounds <= FP_MAX_ROUNDS;
}
inline bool fp_parts_ok(const dppr_forward_push_out_t *o) {
    const uint32_t w = fp_which(o);
    if ((w & FP_TOPK) && !topk_args_ok(o->k, o->min_p, o->topk_ids, o->topk_p, o->topk_counts)) return false;
    if ((w & FP_AT) && !(o->at_ids && (o->at_p || o->at_r) && o->n_at >= 1 && o->n_at <= DPPR_FORWARD_AT_MAX)) return false;
    if ((w & FP_DENSE) && !ex_dense_args_ok(DPPR_DENSE_P, o->dense_dtype, o->dense_layout)) return false;
    return true;
}
// the start sets: the rules of tg_check with the push's own limit on a column. The offsets are checked before any id is read.
inline TgCheck fp_csr_check(const int64_t *offsets, const int32_t *ids, const double *weights, int64_t m, int64_t V) {
    if (m < 1 || m > DPPR_FORWARD_MAX_M) return TG_BAD_N;
    if (!offsets || !ids || !weights) return TG_NULL;
    if (offsets[0] != 0) return TG_BAD_OFFSETS;
    for (int64_t i = 0; i < m; ++i)
        if (offsets[i + 1] < offsets[i]) return TG_BAD_OFFSETS;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n < 1 || n > FP_SET_MAX) return TG_BAD_SIZE;
    }
    for (int64_t i = 0; i < m; ++i)
        if (TgCheck c = tg_check_lane(ids + offsets[i], weights + offsets[i], offsets[i + 1] - offsets[i], V)) return c;
    return TG_OK;
}
inline bool fp_hook_ok(int piece_edges, int team, int chunk_rounds) {
    return fw_hook_ok(piece_edges, team) && chunk_rounds >= 0 && chunk_rounds <= FP_MAX_ROUNDS;
}

// ---- the chunk schedule ----------------------------------------------------------------------------------------------------------
constexpr int fp_chunk(int forced) { return forced > 0 ? forced : FP_CHUNK; }
// the last round of the chunk that starts after round k (k < max_rounds)
constexpr int fp_chunk_end(int k, int max_rounds, int chunk) { return k + chunk < max_rounds ? k + chunk : max_rounds; }
// read-backs of a call that never converges
constexpr int fp_chunks(int max_rounds, int chunk) { return (max_rounds + chunk - 1) / chunk; }

// ---- sizes -----------------------------------------------------------------------------------------------------------------------
constexpr size_t fp_bitmap_words(int64_t V) { return (size_t)((V > 0 ? V : 1) + 31) / 32; }
// a list of rows (front[2], recv[2]): a row enters a list once per round
constexpr size_t fp_list_cap(int64_t V) { return (size_t)(V > 0 ? V : 1); }
// pieces of the out-rows of a frontier: a row of d out-edges has ceil(d / FP_MARK_PIECE) <= d / FP_MARK_PIECE + 1 of them
constexpr long long fp_mark_pieces(long long outdeg) { return (outdeg + FP_MARK_PIECE - 1) / FP_MARK_PIECE; }
constexpr size_t fp_mark_cap(int64_t V, long long Ed) { return (size_t)((V > 0 ? V : 1) + Ed / FP_MARK_PIECE + 1); }
constexpr int fp_grid(long long units, int per_wg) {
    const long long g = (units + per_wg - 1) / per_wg;
    return g < 1 ? 1 : g < FP_GRID_MAX ? (int)g : FP_GRID_MAX;
}

// ---- the work space on the device --------------------------------------------------------------------------------------------------
struct FpHead {                       // zeroed per call
    FwHead fw;                        // what k_fw_pieces reads: frozen stays 0; n_items, n_long, overflow of the round's long receivers
    unsigned last_act;                // bit c: column c pushed in the last round that ran (THE word the host reads back per chunk)
    unsigned act;                     // ... in the round being selected
    unsigned n_front[2], n_recv[2];   // rows of the lists
    unsigned n_mark;                  // queued pieces of the frontier's out-rows
    unsigned overflow;                // a list was too short (never)
    int rounds_used[Q_LANES];
    unsigned long long pushes[Q_LANES], left[Q_LANES];
    unsigned long long work[3];
    double rem[Q_LANES];
};
struct FpSeed {                       // a seed of the table: external id, column, weight; the device answers `row`
    int id, col;
    double w;
    int row, pad;                     // internal id, or -1: no row (answered by the host)
};
static_assert(sizeof(FpSeed) == 24, "a seed of the table is 24 bytes");

// ---- the seeds the host answers --------------------------------------------------------------------------------------------------
// p of a seed without a row: one multiplication
inline double fp_rowless_p(double w) {
    volatile double v = FW_ALPHA * w;
    return v;
}
// (id, p) enters a column's top k -- ids / ps [k], `count` of them filled, p descending, ties by id ascending, p > min_p, entries
// past the count: id -1, p 0.0 -- where the order puts it; the last entry of a full list falls out. Returns the new count.
inline int fp_topk_insert(int32_t *ids, double *ps, int count, int k, double min_p, int32_t id, double p) {
    if (!(p > min_p)) return count;
    int at = 0;
    while (at < count && (ps[at] > p || (ps[at] == p && ids[at] < id))) ++at;
    if (at >= k) return count;
    const int n = count < k ? count + 1 : k;
    for (int j = n - 1; j > at; --j) {
        ids[j] = ids[j - 1];
        ps[j] = ps[j - 1];
    }
    ids[at] = id;
    ps[at] = p;
    return n;
}

// ---- one round on the host ---------------------------------------------------------------------------------------------------------
// One column over an in-CSR by vertex id (ptr [V + 1], tail [ptr[V]]) with out-degrees d [V]: select and push, then the gather over
// EVERY row (the definition). y is scratch [V]. Returns |F|.
inline long long fp_round_ref(int V, const int *ptr, const int *tail, const int *d, double eps, double *p, double *r, double *y, int piece) {
    long long pushed = 0;
    for (int u = 0; u < V; ++u) {
        const double den = (double)(d[u] + 1);
        volatile double thr = eps * den;
        y[u] = 0.0;
        if (r[u] > thr) {
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
