// dppr_explain_plan.hpp -- what the explain queries (dppr_explain_at / dppr_group_explain_at) decide before any device is
// involved: the check of a call's arguments, the layout of the result block (which planes it holds, where, 8-byte alignment of the
// double planes), whether the memo of next hops is used and what it takes, and the grids. Pure host code without HIP includes
// (dppr_host_query.hpp checks a call and lays it out with it, dppr_explain.hpp asserts its constants;
// tests/native/explain_plan_test.cpp drives it on the CPU under the sanitizers).
//
// BLOCK, one copy to the host. Only the planes a call asks for have room; the double planes come first, so every one of them
// starts at a multiple of 8 whatever m, n, f and depth are; the int planes follow; the queried ids, which nobody copies back, last:
//   self [m][n] | nbr_c [m][n][f] | path_p [m][n][depth + 1] | path_c [m][n][depth]            (doubles)
//   deg [m] | distinct [m] | nbr_count [m][n] | nbr [m][n][f] | nbr_mult [m][n][f] | len [m][n] | end [m][n] | path [m][n][depth + 1]
//   <- copy_bytes ->  ids [m]  <- total_bytes
// MEMO. One 64-bit word (next internal id << 32 | mult) per (live row, lane): the arg-max of the contributor order of that pair,
// EX_MEMO_UNKNOWN (all ones, what a memset of 0xff leaves) until some wave has computed it, next = -1 and mult = 0 (never all
// ones) where the order is empty. It lies in the first plane of the scratch state of the ranked family: (live rows) x n words.
#pragma once

#include "dppr_query_plan.hpp"

namespace dppr {

constexpr int EX_BLOCK = 256;                // both kernels: four waves, one (query, lane) pair each
constexpr int EX_PAIR_WAVES = EX_BLOCK / 64;
constexpr int EX_WAVE_ROWS = 64;             // entries of a row a wave takes per step (dppr_debug_explain lowers it)
constexpr unsigned long long EX_MEMO_UNKNOWN = ~0ull;
// The memo pays once its memset and its atomics cost less than the arg-maxes the waves would repeat. profiles/explain_times.md
// has no figure yet that shows such a size, so the plan leaves it off; dppr_debug_explain(memo = 1) turns it on.
constexpr long long EX_MEMO_MIN_PAIRS = -1;  // (query, lane) pairs from which the plan turns the memo on; -1: never

enum : uint32_t { // the outputs of a call, one bit per pointer of dppr_explain_out_t
    EX_DEG = 1u << 0, EX_DISTINCT = 1u << 1, EX_SELF = 1u << 2, EX_NBR_COUNT = 1u << 3, EX_NBR = 1u << 4, EX_NBR_MULT = 1u << 5,
    EX_NBR_C = 1u << 6, EX_LEN = 1u << 7, EX_END = 1u << 8, EX_PATH = 1u << 9, EX_PATH_P = 1u << 10, EX_PATH_C = 1u << 11,
    EX_FIRST = EX_DEG | EX_DISTINCT | EX_SELF | EX_NBR_COUNT | EX_NBR | EX_NBR_MULT | EX_NBR_C, // what k_ex_first writes
    EX_WALK = EX_LEN | EX_END | EX_PATH | EX_PATH_P | EX_PATH_C,                                 // what k_ex_path writes
};

inline uint32_t ex_which(const dppr_explain_out_t *o, int f, int depth) {
    if (!o) return 0;
    uint32_t w = 0;
    if (o->deg) w |= EX_DEG;
    if (o->distinct) w |= EX_DISTINCT;
    if (o->self) w |= EX_SELF;
    if (o->nbr_count) w |= EX_NBR_COUNT;
    if (o->nbr && f > 0) w |= EX_NBR;
    if (o->nbr_mult && f > 0) w |= EX_NBR_MULT;
    if (o->nbr_c && f > 0) w |= EX_NBR_C;
    if (o->len) w |= EX_LEN;
    if (o->end) w |= EX_END;
    if (o->path) w |= EX_PATH;
    if (o->path_p) w |= EX_PATH_P;
    if (o->path_c && depth > 0) w |= EX_PATH_C;
    return w;
}

inline bool ex_args_ok(const int32_t *ids, int32_t m, int32_t f, int32_t depth, int64_t V, const dppr_explain_out_t *out) {
    if (m < 0 || m > DPPR_EXPLAIN_MAX_M) return false;
    if (f < 0 || f > DPPR_EXPLAIN_MAX_F || depth < 0 || depth > DPPR_EXPLAIN_MAX_DEPTH || f + depth < 1) return false;
    if (m > 0 && (!ids || !out)) return false;
    return ids_in_range(ids, m, V);
}
// dppr_debug_explain
inline bool ex_hook_ok(int memo, int wave_rows) { return memo >= -1 && memo <= 1 && wave_rows >= 1 && wave_rows <= EX_WAVE_ROWS; }

struct ExplainLayout {
    size_t off_self = 0, off_nbr_c = 0, off_path_p = 0, off_path_c = 0;
    size_t off_deg = 0, off_distinct = 0, off_nbr_count = 0, off_nbr = 0, off_nbr_mult = 0, off_len = 0, off_end = 0, off_path = 0;
    size_t off_ids = 0;
    size_t copy_bytes = 0, total_bytes = 0;
};
constexpr ExplainLayout ex_layout(int m, int n, int f, int depth, uint32_t which) {
    ExplainLayout l;
    const size_t mn = (size_t)m * (size_t)n;
    size_t at = 0;
    auto take = [&](uint32_t bit, size_t elems, size_t elem_bytes) {
        const size_t here = at;
        if (which & bit) at += elems * elem_bytes;
        return here;
    };
    l.off_self = take(EX_SELF, mn, sizeof(double));
    l.off_nbr_c = take(EX_NBR_C, mn * (size_t)f, sizeof(double));
    l.off_path_p = take(EX_PATH_P, mn * ((size_t)depth + 1), sizeof(double));
    l.off_path_c = take(EX_PATH_C, mn * (size_t)depth, sizeof(double));
    l.off_deg = take(EX_DEG, (size_t)m, sizeof(int32_t));
    l.off_distinct = take(EX_DISTINCT, (size_t)m, sizeof(int32_t));
    l.off_nbr_count = take(EX_NBR_COUNT, mn, sizeof(int32_t));
    l.off_nbr = take(EX_NBR, mn * (size_t)f, sizeof(int32_t));
    l.off_nbr_mult = take(EX_NBR_MULT, mn * (size_t)f, sizeof(int32_t));
    l.off_len = take(EX_LEN, mn, sizeof(int32_t));
    l.off_end = take(EX_END, mn, sizeof(int32_t));
    l.off_path = take(EX_PATH, mn * ((size_t)depth + 1), sizeof(int32_t));
    l.copy_bytes = at;
    l.off_ids = at;
    l.total_bytes = pad8(at + sizeof(int32_t) * (size_t)m);
    if (l.total_bytes < 8) l.total_bytes = 8; // (a buffer of no bytes is not one)
    return l;
}

// forced: dppr_debug_explain (-1: the plan decides). A call without a path has no use for it.
constexpr bool ex_memo_on(int m, int n, int depth, uint32_t which, int forced) {
    if (depth < 1 || !(which & EX_WALK) || m < 1) return false;
    if (forced >= 0) return forced != 0;
    return EX_MEMO_MIN_PAIRS >= 0 && (long long)m * n >= EX_MEMO_MIN_PAIRS;
}
constexpr size_t ex_memo_elems(size_t live_rows, int n) { return (live_rows > 0 ? live_rows : 1) * (size_t)n; }

// one wave per (query, lane)
constexpr int ex_grid(int m, int n) {
    const long long pairs = (long long)m * n;
    return pairs < 1 ? 1 : (int)((pairs + EX_PAIR_WAVES - 1) / EX_PAIR_WAVES);
}

} // namespace dppr
