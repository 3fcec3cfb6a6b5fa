// dppr_changes.hpp -- what a batch moved: a MARK of p per source and the top k of |p - mark| (dppr_mark / dppr_group_mark,
// dppr_changes / dppr_group_changes). Never called from the update path.
//
// MARK. A copy of p as it was at dppr_mark, [V][gw] doubles indexed by EXTERNAL id (a vertex that had no id then: 0.0). The
// state's rows move when a parked vertex is revived and are permuted by a renumbering; the mark does neither, so neither
// flush_moves nor the renumbering knows about it, and a result never depends on the numbering. The price is one gathered line
// per occupied row in k_ch_delta.
//
// DELTA. d = p - mark, one subtraction rounded to nearest (__dsub_rn: nothing for the compiler to re-associate or fuse).
//
// SHAPE: materialised, as dppr_wquery.hpp. k_ch_delta streams the occupied rows once -- the live zone [0, n_int), then the parked
// zone -- and writes |d| and d of every lane into two COMPACTED scratch states abs[c * n + lane], d[c * n + lane], c = 0 .. rows - 1,
// with the external id of compacted row c beside them. The selection of dppr_topk.hpp then runs over the scratch as a state of n
// lanes, rows n doubles wide, without a parked zone: TkState::p is |d| (a positive double wherever it qualifies: |d| > min_delta
// >= 0), TkState::r is d, which k_tk_rank delivers next to the ids. Its kernels are used as they are. k_ch_gather fills the
// current p at the result ids. In the same pass k_ch_delta counts the qualifying entries of every lane (LDS, then one global
// atomic per lane and workgroup) and, for a re-mark, stores p into the mark row it has just read.
//
// k_ch_delta: one tile of dppr_topk.hpp per step (its rows, block and padded LDS rows; the bank argument is there). It keeps a load
// loop of its own, not tk_stage_tile: the p row and the mark row of a vertex are read in ONE iteration, so that both loads are in
// flight together and a re-mark stores the p it holds in registers -- with p staged first and the mark gathered in a second loop
// the query measured 3 % slower (profiles/query_layer_refactor_times.md). 16-byte loads where a row is an even number of doubles
// (every group), 8-byte loads on a single-source slot (gw = 1); |d| and d leave with consecutive threads at consecutive addresses.
// Every store is an ordinary vector store; the counters are LDS / global vector atomics.
#pragma once

#include "dppr_changes_plan.hpp"
#include "dppr_topk.hpp"

namespace dppr {

constexpr int CH_BLOCK = 256;                // k_ch_mark, k_ch_gather

// mark[ext * gw + lane] = p of the row that holds ext, 0.0 for a vertex without an id: one pass over the external ids
__global__ __launch_bounds__(CH_BLOCK) void k_ch_mark(const double *__restrict__ p, int gw, const int *__restrict__ ext2int, int V,
                                                      double *__restrict__ mark) {
    const int64_t total = (int64_t)V * gw;
    for (int64_t t = (int64_t)blockIdx.x * CH_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * CH_BLOCK) {
        const int ext = (int)(t / gw), lane = (int)(t % gw);
        const int row = ext2int[ext];
        mark[t] = row >= 0 ? p[(size_t)row * gw + lane] : 0.0;
    }
}

// st: the state (rows of gw doubles, n lanes in use). i2e: external id of every occupied row. mark: [V][gw].
// abs_c, d_c: [st.rows][n], ext_c: [st.rows], moved: [n] (zeroed by the caller).
__global__ __launch_bounds__(TK_TILE_BLOCK) void k_ch_delta(TkState st, const int *__restrict__ i2e, double *__restrict__ mark, int V,
                                                            double min_delta, int remark, double *__restrict__ abs_c,
                                                            double *__restrict__ d_c, int *__restrict__ ext_c, int *__restrict__ moved) {
    __shared__ double s_p[TK_TILE_ROWS * TK_TILE_LDS_ROW];
    __shared__ double s_m[TK_TILE_ROWS * TK_TILE_LDS_ROW];
    __shared__ int s_ext[TK_TILE_ROWS];
    __shared__ int s_cnt[CH_LANES];
    if (threadIdx.x < CH_LANES) s_cnt[threadIdx.x] = 0;
    const int ls = st.gw + 1, half = st.gw / 2;
    const int n_tiles = (st.rows + TK_TILE_ROWS - 1) / TK_TILE_ROWS;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int c0 = tile * TK_TILE_ROWS, cnt = min(TK_TILE_ROWS, st.rows - c0);
        __syncthreads(); // (the subtractions of the previous tile are over; the counters are cleared)
        for (int rl = threadIdx.x; rl < cnt; rl += TK_TILE_BLOCK) {
            const int ext = i2e[tk_row(st, c0 + rl)];
            s_ext[rl] = ext;
            ext_c[c0 + rl] = ext;
        }
        __syncthreads();
        if (st.gw & 1) { // a single-source slot: rows of one double
            for (int j = threadIdx.x; j < cnt * st.gw; j += TK_TILE_BLOCK) {
                const int rl = j / st.gw, l = j % st.gw, ext = s_ext[rl];
                const double v = st.p[(size_t)tk_row(st, c0 + rl) * st.gw + l];
                double m = 0.0;
                if ((unsigned)ext < (unsigned)V) { // (every occupied row holds a vertex; a row that does not has mark 0)
                    double *mp = mark + (size_t)ext * st.gw + l;
                    m = *mp;
                    if (remark) *mp = v;
                }
                s_p[rl * ls + l] = v;
                s_m[rl * ls + l] = m;
            }
        } else {
            for (int j = threadIdx.x; j < cnt * half; j += TK_TILE_BLOCK) {
                const int rl = j / half, h = j % half, ext = s_ext[rl];
                const double2 v = *reinterpret_cast<const double2 *>(st.p + (size_t)tk_row(st, c0 + rl) * st.gw + 2 * h);
                double2 m = make_double2(0.0, 0.0);
                if ((unsigned)ext < (unsigned)V) {
                    double2 *mp = reinterpret_cast<double2 *>(mark + (size_t)ext * st.gw + 2 * h);
                    m = *mp;
                    if (remark) *mp = v;
                }
                s_p[rl * ls + 2 * h] = v.x;
                s_p[rl * ls + 2 * h + 1] = v.y;
                s_m[rl * ls + 2 * h] = m.x;
                s_m[rl * ls + 2 * h + 1] = m.y;
            }
        }
        __syncthreads();
        for (int o = threadIdx.x; o < cnt * st.n; o += TK_TILE_BLOCK) {
            const int rl = o / st.n, lane = o % st.n;
            const double d = __dsub_rn(s_p[rl * ls + lane], s_m[rl * ls + lane]);
            const double a = fabs(d);
            abs_c[(size_t)c0 * st.n + o] = a;
            d_c[(size_t)c0 * st.n + o] = d;
            if (a > min_delta) atomicAdd(&s_cnt[lane], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < st.n && s_cnt[threadIdx.x]) atomicAdd(&moved[threadIdx.x], s_cnt[threadIdx.x]);
}

// the current p at the result ids: one thread per (lane, rank); res_id and out_p are [n][k], entries past a count hold id -1
__global__ __launch_bounds__(CH_BLOCK) void k_ch_gather(const double *__restrict__ p, int gw, int n, int k,
                                                        const int *__restrict__ ext2int, const int *__restrict__ res_id,
                                                        double *__restrict__ out_p) {
    const int total = n * k;
    for (int t = blockIdx.x * CH_BLOCK + threadIdx.x; t < total; t += gridDim.x * CH_BLOCK) {
        const int lane = t / k, ext = res_id[t];
        const int row = ext >= 0 ? ext2int[ext] : -1;
        out_p[t] = row >= 0 ? p[(size_t)row * gw + lane] : 0.0;
    }
}

} // namespace dppr
