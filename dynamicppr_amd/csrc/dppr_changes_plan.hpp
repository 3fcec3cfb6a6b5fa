// dppr_changes_plan.hpp -- the result block of dppr_changes / dppr_group_changes and the checks of their arguments. Pure host code
// without HIP includes (dppr_host_query.hpp lays the device and the pinned block out with it and checks a call with
// it; tests/native/changes_test.cpp drives it on the CPU against a plain restatement).
//
// One block holds everything a call returns, so that one copy brings it to the host:
//     [16 counts][16 moved][ids n x k, padded to 8 bytes][delta n x k][p n x k]   <- copied (copy_bytes)
//     [|delta| n x k]                                                             <- device only (k_tk_rank writes it; not returned)
#pragma once

#include "dppr_query_plan.hpp"

namespace dppr {

constexpr int CH_LANES = Q_LANES;      // (the name the kernels of dppr_changes.hpp know the lane count by)
constexpr int CH_K_MAX = DPPR_TOPK_MAX; // (... and tests/native/changes_test.cpp the largest k)

struct ChLayout {
    size_t off_cnt = 0, off_moved = 0, off_ids = 0, off_delta = 0, off_p = 0, off_abs = 0;
    size_t copy_bytes = 0;  // what comes back to the host: everything in front of off_abs
    size_t total_bytes = 0; // the block on the device
};

constexpr ChLayout ch_layout(int n, int k) {
    ChLayout l;
    const size_t nk = (size_t)n * (size_t)k;
    l.off_cnt = 0;
    l.off_moved = l.off_cnt + sizeof(int) * CH_LANES;
    l.off_ids = l.off_moved + sizeof(int) * CH_LANES;
    l.off_delta = l.off_ids + pad8(sizeof(int) * nk);
    l.off_p = l.off_delta + sizeof(double) * nk;
    l.off_abs = l.off_p + sizeof(double) * nk;
    l.copy_bytes = l.off_abs;
    l.total_bytes = l.off_abs + sizeof(double) * nk;
    return l;
}

// the arguments of a call that do not depend on the engine: k in [1, CH_K_MAX], min_delta >= 0 (false for NaN), the three
// outputs that may not be NULL
inline bool ch_args_ok(int k, double min_delta, const void *ids, const void *delta, const void *counts) {
    return k >= 1 && k <= CH_K_MAX && min_delta >= 0.0 && ids && delta && counts;
}

} // namespace dppr
