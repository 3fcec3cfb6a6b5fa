// dppr_wquery.hpp -- queries of a source group as a weighted set of targets (dppr_group_topk_weighted, dppr_group_score_at).
// Never called from the update path.
//
// SCORE. For query j and a row of the group's state (p_0 .. p_{n-1}, lanes n .. gw-1 are padding):
//     acc = w[j][0] * p_0;   acc = acc + w[j][i] * p_i   for i = 1 .. n-1 in that order
// every product and every sum rounded to double, nothing fused (wq_fold: explicit round-to-nearest multiply and add, which the
// compiler never contracts, whatever -ffp-contract says). A one-hot w[j] therefore returns p_i bit for bit (0 * p is +-0 and
// x + +-0 = x for x != 0; a p of +-0 gives a score of +-0, which never qualifies).
//
// SHAPE: materialised. k_wq_scores streams the occupied rows once -- the live zone [0, n_int) and the parked zone, the rows
// dppr_topk.hpp scans -- and writes the q scores of each into a COMPACTED scratch state score[c * q + j], c = 0 .. rows - 1,
// together with the external id of compacted row c (the tie order needs the ids of the STATE's rows: the lookup follows the
// compaction). The selection of dppr_topk.hpp then runs over the scratch as a state of q lanes, rows q doubles wide, without
// a parked zone: its kernels are used as they are. DESIGN.md section 9c has the byte counts of this shape and of the fused one.
//
// k_wq_scores: one tile of dppr_topk.hpp (tk_stage_tile) per step, then one thread per (row, query): the fold over the staged row.
// Scores leave with consecutive threads at consecutive addresses.
#pragma once

#include "dppr_topk.hpp"

namespace dppr {

constexpr int WQ_BLOCK = 256;                     // k_score_at
constexpr int WQ_LANES = 16;                      // sources of a group, weight vectors of a call (GS_MAX)

// the fold of the header over n consecutive weights and n consecutive doubles of a row
__device__ __forceinline__ double wq_fold(const double *w, const double *p, int n) {
    double acc = __dmul_rn(w[0], p[0]);
    for (int i = 1; i < n; ++i) acc = __dadd_rn(acc, __dmul_rn(w[i], p[i]));
    return acc;
}

// st: the group's state. w: [q][n] on the device. score: [st.rows][q], ext_c: [st.rows].
__global__ __launch_bounds__(TK_TILE_BLOCK) void k_wq_scores(TkState st, const int *__restrict__ i2e, const double *__restrict__ w,
                                                             int q, double *__restrict__ score, int *__restrict__ ext_c) {
    __shared__ double s_w[WQ_LANES * WQ_LANES];
    __shared__ double s_p[TK_TILE_ROWS * TK_TILE_LDS_ROW];
    for (int i = threadIdx.x; i < q * st.n; i += TK_TILE_BLOCK) s_w[i] = w[i];
    const int ls = st.gw + 1;
    const int n_tiles = (st.rows + TK_TILE_ROWS - 1) / TK_TILE_ROWS;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int c0 = tile * TK_TILE_ROWS, cnt = min(TK_TILE_ROWS, st.rows - c0);
        __syncthreads(); // (the folds of the previous tile are over; the weights are in place)
        tk_stage_tile(st, i2e, c0, cnt, s_p, ext_c, [](int, int, int) {});
        __syncthreads();
        for (int o = threadIdx.x; o < cnt * q; o += TK_TILE_BLOCK) {
            const int rl = o / q, j = o % q;
            score[(size_t)c0 * q + o] = wq_fold(s_w + j * st.n, s_p + rl * ls, st.n);
        }
    }
}

// scores at m external ids: one thread per (id, query); out [m][q]. A vertex without an internal id folds n zeros (the sign of
// the result follows the weights, as the definition says).
__global__ __launch_bounds__(WQ_BLOCK) void k_score_at(const double *__restrict__ p, int gw, int n, const int *__restrict__ ext2int,
                                                       const int *__restrict__ ids, int m, const double *__restrict__ w, int q,
                                                       double *__restrict__ out) {
    __shared__ double s_w[WQ_LANES * WQ_LANES];
    for (int i = threadIdx.x; i < q * n; i += WQ_BLOCK) s_w[i] = w[i];
    __syncthreads();
    const int64_t total = (int64_t)m * q;
    for (int64_t t = (int64_t)blockIdx.x * WQ_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * WQ_BLOCK) {
        const int i = (int)(t / q), j = (int)(t % q);
        const int row = ext2int[ids[i]];
        double v[WQ_LANES];
#pragma unroll
        for (int s = 0; s < WQ_LANES; ++s) v[s] = (s < n && row >= 0) ? p[(size_t)row * gw + s] : 0.0;
        double acc = __dmul_rn(s_w[j * n], v[0]);
#pragma unroll
        for (int s = 1; s < WQ_LANES; ++s)
            if (s < n) acc = __dadd_rn(acc, __dmul_rn(s_w[j * n + s], v[s]));
        out[t] = acc;
    }
}

} // namespace dppr
