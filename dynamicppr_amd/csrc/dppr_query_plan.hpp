// dppr_query_plan.hpp -- what the state queries share before any device is involved: the public constants (include/dppr.h, by
// inclusion: no query header restates them), the lane count of a group, the 8-byte padding of a block's sections, the check that
// every id lies in [0, V), the argument checks of top-k, the point reads and the weighted forms, and the result blocks of
// dppr_topk / dppr_read_at / dppr_group_score_at. Pure host code without HIP includes (the plan headers of the other families
// include it, dppr_host_query.hpp checks a call and lays its blocks out with it; tests/native/query_plan_test.cpp drives it on
// the CPU against plain restatements).
//
// BLOCK of a top-k call, one copy to the host:
//     [16 counts]  <- TK_OFF_IDS = 64 bytes    [ids n x k, padded to 8 bytes][p n x k][r n x k]
// r is always written on the device and copied only when the caller asked for it.
// BUFFER of a point read: [ids m, padded to 8 bytes][out m x cols], and a second [out m x cols] for dppr_read_at (p, then r).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/dppr.h"

namespace dppr {

constexpr int Q_LANES = 16; // sources of a group: GS_MAX of dppr_multi.hpp (asserted equal in dppr_host_query.hpp)

constexpr size_t pad8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

// every id inside [0, V)? (m <= 0: nothing is read)
inline bool ids_in_range(const int32_t *ids, int64_t m, int64_t V) {
    for (int64_t i = 0; i < m; ++i)
        if (ids[i] < 0 || ids[i] >= V) return false;
    return true;
}

inline bool topk_args_ok(int32_t k, double min_p, const void *ids, const void *p, const void *cnt) {
    return k >= 1 && k <= DPPR_TOPK_MAX && min_p >= 0.0 && ids && p && cnt; // (min_p >= 0 is false for NaN)
}
inline bool read_at_args_ok(const int32_t *ids, int32_t m, int64_t V) {
    return m >= 0 && (m == 0 || ids) && ids_in_range(ids, m, V);
}
// weights [q][n]: q in [1, 16], every entry finite
inline bool weights_ok(const double *w, int32_t q, int n) {
    if (!w || q < 1 || q > Q_LANES) return false;
    for (int i = 0; i < q * n; ++i)
        if (!std::isfinite(w[i])) return false;
    return true;
}

constexpr size_t TK_OFF_IDS = 64; // the 16 counts come first

struct TkLayout {
    size_t off_cnt = 0, off_ids = TK_OFF_IDS, off_p = 0, off_r = 0;
    size_t copy_bytes = 0;  // what comes back to the host: r only where it was asked for
    size_t total_bytes = 0; // the block on the device
};

constexpr TkLayout tk_layout(int n, int k, bool with_r) {
    TkLayout l;
    const size_t nk = (size_t)n * (size_t)k;
    l.off_p = l.off_ids + pad8(sizeof(int32_t) * nk);
    l.off_r = l.off_p + sizeof(double) * nk;
    l.total_bytes = l.off_r + sizeof(double) * nk;
    l.copy_bytes = with_r ? l.total_bytes : l.off_r;
    return l;
}

// The compacted scratch state of the weighted, changes and ranked queries: one or two planes of [occupied rows][lanes] doubles
// and the external id of every row (a state without an occupied row still has room for one)
constexpr size_t scratch_plane_elems(size_t rows, int lanes) { return (rows > 0 ? rows : 1) * (size_t)lanes; }
constexpr size_t scratch_ext_elems(size_t rows) { return rows > 0 ? rows : 1; }

struct RaLayout {
    size_t off_ids = 0, off_a = 0, off_b = 0; // off_b: the second output of a call that has two
    size_t total_bytes = 0;
};

// m ids and `outs` (1 or 2) outputs of m x cols doubles
constexpr RaLayout ra_layout(int m, int cols, int outs) {
    RaLayout l;
    l.off_a = pad8(sizeof(int32_t) * (size_t)m);
    l.off_b = l.off_a + sizeof(double) * (size_t)m * (size_t)cols;
    l.total_bytes = l.off_a + (size_t)outs * sizeof(double) * (size_t)m * (size_t)cols;
    return l;
}

} // namespace dppr
