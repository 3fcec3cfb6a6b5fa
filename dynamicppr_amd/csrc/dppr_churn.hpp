// dppr_churn.hpp -- a running source group changes its sources (dppr_group_replace_source / dppr_group_add_source /
// dppr_group_remove_source): the device work that re-shapes the interleaved [V][gw] rows of dppr_multi.hpp. The reference
// has no counterpart (one source per process, gpu/PPRGPU.cuh:24; its Init, gpu/PPRCommon.cuh:12-22, is what one column
// receives here).
//
// Both kernels run BETWEEN two frontier loops of a converged group and cover all V rows, the live and the parked zone
// alike: no activity bit is set, so the snapshot rows x / x2 mean nothing and are neither read nor initialised (a width
// change simply allocates them afresh), and p / r are complete. Neither kernel sets a bit, uses an atomic, LDS or
// inline assembly: both are streaming passes.
//   k_gcol_init  one lane of every row becomes a from-scratch source: p = 0, r = e_src. The other lanes of a row are
//                not touched (8 bytes written per row and array: the stride is the price of the interleaving).
//   k_grow_remap out of place, rows of gw_old doubles -> rows of gw_new doubles, new lane j' taking old lane map[j']
//                (-1: zero). One thread per DESTINATION double: consecutive lanes write consecutive doubles, and the
//                reads of a wave fall into the same few consecutive source rows.
#pragma once

#include "dppr_churn_plan.hpp"
#include "dppr_common.hpp"

namespace dppr {

struct ColMap {
    int m[CHURN_LANES]; // destination lane -> source lane, -1 = zeros
};

// Init (gpu/PPRCommon.cuh:12-22) for ONE state lane: p[v][lane] = 0, r[v][lane] = (v == src). One thread per vertex.
__global__ __launch_bounds__(BLOCK) void k_gcol_init(double *__restrict__ p, double *__restrict__ r, int V, int gw, int lane, int src) {
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * BLOCK) {
        const int64_t i = v * gw + lane;
        p[i] = 0.0;
        r[i] = v == src ? 1.0 : 0.0;
    }
}

// dst[v][j'] = map[j'] >= 0 ? src[v][map[j']] : 0.0 for all V rows. A workgroup pass covers BLOCK / gw_new whole rows:
// thread t owns lane t % gw_new of row t / gw_new of every pass (both fixed for the thread, so the map is looked up
// once), and the threads of a pass write one contiguous run of rows * gw_new doubles. Element indices are 64-bit
// (V * 16 doubles passes 2^31 on a friendster-size id range).
__global__ __launch_bounds__(BLOCK) void k_grow_remap(double *__restrict__ dst, const double *__restrict__ src, int V, int gw_new, int gw_old,
                                                      ColMap map) {
    const int rows = BLOCK / gw_new; // rows per workgroup pass (gw_new <= 16: at least 16)
    const int row = (int)threadIdx.x / gw_new, j = (int)threadIdx.x % gw_new;
    if (row >= rows) return; // (BLOCK is no multiple of 6, 10, 12, 14: the last few threads have no row)
    const int from = map.m[j];
#pragma unroll 4
    for (int64_t v = (int64_t)blockIdx.x * rows + row; v < V; v += (int64_t)gridDim.x * rows)
        dst[v * gw_new + j] = from >= 0 ? src[v * gw_old + from] : 0.0;
}

} // namespace dppr
