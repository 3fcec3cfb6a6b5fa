// dppr_targets.hpp -- weighted vertex sets as the targets of a source group: the device side of dppr_add_target_group /
// dppr_group_replace_target. A lane's seed vector h replaces the indicator e_s of the reference's Init (gpu/PPRCommon.cuh:12-22)
// and of the stream update's add expression (gpu/StreamUpdate.cuh:50-72); the invariant a lane keeps is
//     p[u] + ALPHA * r[u] == ALPHA * h[u] + (1 - ALPHA) / (outdeg(u) + 1) * sum over v in out(u) of p[v]
// and nothing else of the engine knows h: seeding, sweeps, the push tail and every query read p / r rows only.
//
// The seed table of a group (dppr_targets_plan.hpp lays it out and builds it on the host): lane offsets [17], internal ids
// ascending within a lane, weights. TgDev is the three pointers into that one block.
//   tg_h          h of a lane at a vertex: binary search in the lane's slice, 0.0 when the vertex is no seed (at most 17 steps
//                 for DPPR_TARGET_SET_MAX seeds; called once per tail run by the stream update, dppr_update.hpp)
//   k_tg_init     p = 0, r = 0 for all lanes of all V rows, one streaming pass (the group's Init, first half)
//   k_tg_col_init the same for one lane (a lane of a running group is replaced or added, dppr_churn.hpp)
//   k_tg_scatter  r[seed][lane] = weight for the seeds of lanes [lane0, lane1): the second, tiny launch of either
// No atomic, no LDS, no inline assembly: plain loads and vector stores. Every seed id is checked against V before its row is
// written.
#pragma once

#include "dppr_common.hpp"
#include "dppr_targets_plan.hpp"

namespace dppr {

struct TgDev {
    const double *w; // [total]
    const int *off;  // [TG_LANES + 1]
    const int *ids;  // [total] internal ids, ascending within a lane
};

__device__ __forceinline__ double tg_h(const TgDev &t, int lane, int v) {
    const int end = t.off[lane + 1];
    int lo = t.off[lane], hi = end;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (t.ids[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo < end && t.ids[lo] == v ? t.w[lo] : 0.0;
}

__global__ __launch_bounds__(BLOCK) void k_tg_init(double *__restrict__ p, double *__restrict__ r, int V, int gw) {
    const int64_t n = (int64_t)V * gw;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        p[i] = 0.0;
        r[i] = 0.0;
    }
}

__global__ __launch_bounds__(BLOCK) void k_tg_col_init(double *__restrict__ p, double *__restrict__ r, int V, int gw, int lane) {
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * BLOCK) {
        const int64_t i = v * gw + lane;
        p[i] = 0.0;
        r[i] = 0.0;
    }
}

// One thread per seed of lanes [lane0, lane1). A seed's lane: the last lane whose slice starts at or before it (empty lanes
// share a start with their successor and are skipped by the `<=`).
__global__ __launch_bounds__(BLOCK) void k_tg_scatter(double *__restrict__ r, int V, int gw, TgDev t, int lane0, int lane1) {
    const int a = t.off[lane0], b = t.off[lane1];
    for (int k = a + blockIdx.x * BLOCK + threadIdx.x; k < b; k += gridDim.x * BLOCK) {
        int lane = lane0;
        while (lane + 1 < lane1 && t.off[lane + 1] <= k) ++lane;
        const int v = t.ids[k];
        if (v >= 0 && v < V && lane < gw) r[(int64_t)v * gw + lane] = t.w[k];
    }
}

} // namespace dppr
