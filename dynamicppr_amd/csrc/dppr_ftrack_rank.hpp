// dppr_ftrack_rank.hpp -- the ranked, position and sample queries over a forward track (dppr_ftrack_topk_ranked /
// dppr_ftrack_rank_score_at / dppr_ftrack_position_at / dppr_ftrack_sample): THE SCORE of dppr_rank.hpp (rk_score / rk_factor /
// rk_masked_out: the one score function) applied to a track's p, read IN PLACE from the track's [V][gw] plane by EXTERNAL id --
// no load into the forward family's planes, so a seed without a row is where it is in dppr_ftrack_read. Never called from the
// update path. include/dppr.h states every output; dppr_ftrack_rank_plan.hpp has the steps of a call.
//
// SHAPE.
//   k_fr_rowlen   one thread per seed of the call: the lengths of its live out-row and in-row (0 without a live row), for the
//                 host's piece list (rk_pieces of dppr_rank_plan.hpp).
//   k_fr_mark     one wave per piece: the entries read coalesced, the neighbour's external id through int2ext, bit `column` of
//                 excl[ext] set by one 32-bit vector atomic OR whose return value is not used; the seeds' own bits by one thread
//                 per seed, row or no row. excl is one word per EXTERNAL id, zeroed per call. An OR does not depend on the order
//                 in which the pieces arrive.
//   k_fr_count    a tile of tile_rows external ids per step of a workgroup, walked in stages of at most FR_STAGE ids: the rows of
//                 the plane staged in LDS with 16-byte loads (a tile is one contiguous run of the plane; gw is even), rows padded
//                 by one double; a thread per id fetches the mask byte, the factor (a DEV gather by external id, the degree
//                 through ext2int -> out_row_ptr) and the exclusion word, then KEEPS the id iff some column has
//                 score > min_score. The kept ids of a tile are counted by a ballot and a popcount per wave, the waves in LDS.
//   (scan)        k_ex_scan of dppr_export.hpp over the tiles' counts as one lane: the first row of every tile, the total.
//   k_fr_fill     the same stages and the same scores again; a kept id's row is base[tile] + the kept ids before it in the tile
//                 (earlier stages, earlier waves, mbcnt of the ballot): ascending external id, no position from an atomic. The
//                 scores leave (row, column) by (row, column) into the COMPACTED scratch state score[row * m + col] with
//                 ext_c[row] -- the layout the selection of dppr_topk.hpp and k_pos_count consume as they are.
//   k_fr_score_at one thread per (id, column), straight from the plane.
//   k_fr_leaves   the sibling of k_sm_leaves (dppr_sample.hpp): the weights of a subtile from the plane by external id, then the
//                 shared sm_subtile_out / sm_tile_nodes. The upper levels and both draw forms follow as they are.
// A row dropped by the compaction has no column with score > min_score: it is in no top-k, precedes no position and joins no count.
// DESIGN.md section 9v has the byte counts of this shape.
#pragma once

#include "dppr_common.hpp"
#include "dppr_ftrack_rank_plan.hpp"
#include "dppr_rank.hpp"
#include "dppr_sample.hpp"

namespace dppr {

static_assert(FR_BLOCK == 4 * WAVE && FR_STAGE == FR_BLOCK && FR_LDS_ROW == GS_MAX + 1 && FR_SCAN_LANES == WAVE && SM_SUB == FR_BLOCK,
              "dppr_ftrack_rank_plan.hpp restates the wave and the lanes");

struct FrTrack { // a track as the kernels read it
    const double *p;         // [V][gw] by external id
    int gw, m, V;
    const int *ext2int;      // [V]
};

// ---- marking by external id --------------------------------------------------------------------------------------------------
// len [total][2]: out-row, in-row of the seed's live row
__global__ __launch_bounds__(FR_BLOCK) void k_fr_rowlen(FrSeeds s, const int *__restrict__ ids, const int *__restrict__ ext2int, RkGraph g,
                                                        int *__restrict__ len) {
    const int total = s.off[GS_MAX];
    for (int pos = blockIdx.x * FR_BLOCK + threadIdx.x; pos < total; pos += gridDim.x * FR_BLOCK) {
        const int ext = ids[pos];
        const int u = (unsigned)ext < (unsigned)g.V ? ext2int[ext] : -1;
        const bool ok = (unsigned)u < (unsigned)g.n_int;
        len[2 * (size_t)pos] = ok ? g.out_row_ptr[u + 1] - g.out_row_ptr[u] : 0;
        len[2 * (size_t)pos + 1] = ok ? g.in_row_ptr[u + 1] - g.in_row_ptr[u] : 0;
    }
}

// items: the piece list (cl_item: position | direction | chunk). excl [V] by external id, zeroed by the caller.
__global__ __launch_bounds__(FR_BLOCK) void k_fr_mark(FrSeeds s, const int *__restrict__ ids, const int *__restrict__ ext2int,
                                                      const int *__restrict__ int2ext, RkGraph g, unsigned flags, int piece,
                                                      const unsigned long long *__restrict__ items, unsigned n_items, unsigned *__restrict__ excl) {
    for (unsigned t = blockIdx.x * FR_WAVES + wave_id(); t < n_items; t += gridDim.x * FR_WAVES) {
        const unsigned long long it = items[t];
        const int pos = (int)cl_item_pos(it), dir = (int)cl_item_dir(it);
        if (pos >= s.off[GS_MAX]) continue;
        const int col = __builtin_amdgcn_readfirstlane(fr_col_of(s, pos));
        const int ext = __builtin_amdgcn_readfirstlane(ids[pos]);
        if ((unsigned)ext >= (unsigned)g.V) continue;
        const int u = __builtin_amdgcn_readfirstlane(ext2int[ext]);
        if ((unsigned)u >= (unsigned)g.n_int) continue; // (no live row: no piece was made)
        const int *rp = dir ? g.in_row_ptr : g.out_row_ptr;
        const int r0 = __builtin_amdgcn_readfirstlane(rp[u]), r1 = __builtin_amdgcn_readfirstlane(rp[u + 1]);
        const long long lo = (long long)r0 + (long long)cl_item_chunk(it) * piece;
        const long long hi = min((long long)r1, lo + piece);
        const unsigned bit = 1u << col;
        for (long long e = lo + lane_id(); e < hi; e += WAVE) {
            const int w = dir ? g.in_adj[e].v : ld_stream(g.out_col + e);
            if ((unsigned)w >= (unsigned)g.n_int) continue;
            const int we = int2ext[w];
            if ((unsigned)we < (unsigned)g.V) atomicOr(&excl[we], bit);
        }
    }
    if (flags & DPPR_EXCLUDE_SEEDS) {
        const int total = s.off[GS_MAX];
        for (int pos = blockIdx.x * FR_BLOCK + threadIdx.x; pos < total; pos += gridDim.x * FR_BLOCK) {
            const int ext = ids[pos];
            if ((unsigned)ext < (unsigned)g.V) atomicOr(&excl[ext], 1u << fr_col_of(s, pos)); // (row or no row)
        }
    }
}

// ---- the stage of the count / fill passes ------------------------------------------------------------------------------------
// External ids [e0, e0 + cnt) of the plane into s_p (row rl at s_p + rl * (gw + 1)): the ids are consecutive rows of the plane,
// so consecutive threads load consecutive 16 bytes. Thread rl < cnt fetches what the id's own data decide. The caller
// synchronises before it reads.
template <int KIND, class T>
__device__ __forceinline__ void fr_stage(const FrTrack &tk, const unsigned *__restrict__ excl, const RkRule &rule, const RkGraph &g, long long e0,
                                         int cnt, double *s_p, double *s_f, unsigned *s_x) {
    const int ls = tk.gw + 1, half = tk.gw / 2;
    const double2 *src = reinterpret_cast<const double2 *>(tk.p + (size_t)e0 * tk.gw); // (gw even: every row starts on 16 bytes)
    for (int j = threadIdx.x; j < cnt * half; j += FR_BLOCK) {
        const int rl = j / half, h = j % half;
        const double2 v = src[j];
        s_p[rl * ls + 2 * h] = v.x;
        s_p[rl * ls + 2 * h + 1] = v.y;
    }
    const int rl = threadIdx.x;
    if (rl < cnt) {
        const int ext = (int)(e0 + rl);
        unsigned x = excl ? excl[ext] : 0u;
        if (rk_masked_out(rule, ext)) x = 0xffffffffu;
        s_x[rl] = x;
        s_f[rl] = rk_factor<KIND, T>(rule, g, ext, tk.ext2int[ext]);
    }
}
// does staged row rl keep its id: some column with score > min_score (false for a NaN)
template <int KIND>
__device__ __forceinline__ bool fr_keeps(const double *s_p, const double *s_f, const unsigned *s_x, int ls, int m, int rl, double min_score) {
    bool keep = false;
    const double f = s_f[rl];
    const unsigned x = s_x[rl];
    for (int c = 0; c < m; ++c) keep = keep || rk_score<KIND>(s_p[rl * ls + c], f, (x >> c) & 1u) > min_score;
    return keep;
}

// cnt [tiles]: the kept ids of every tile
template <int KIND, class T>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_count(FrTrack tk, const unsigned *__restrict__ excl, RkRule rule, RkGraph g, double min_score,
                                                       int tile_rows, int *__restrict__ cnt) {
    __shared__ double s_p[FR_STAGE * FR_LDS_ROW];
    __shared__ double s_f[FR_STAGE];
    __shared__ unsigned s_x[FR_STAGE];
    __shared__ int s_cnt[FR_WAVES];
    const int ls = tk.gw + 1, stage = fr_stage_rows(tile_rows);
    const long long tiles = fr_tiles(tk.V, tile_rows);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long t0 = fr_tile_first(tile, tile_rows), t1 = t0 + fr_tile_count(tile, tk.V, tile_rows);
        int kept = 0; // (of this wave, over the stages)
        for (long long e0 = t0; e0 < t1; e0 += stage) {
            const int n = (int)min((long long)stage, t1 - e0);
            __syncthreads(); // (the previous stage is read)
            fr_stage<KIND, T>(tk, excl, rule, g, e0, n, s_p, s_f, s_x);
            __syncthreads();
            const bool keep = (int)threadIdx.x < n && fr_keeps<KIND>(s_p, s_f, s_x, ls, tk.m, threadIdx.x, min_score);
            kept += __popcll(__ballot(keep));
        }
        if (lane_id() == 0) s_cnt[wave_id()] = kept;
        __syncthreads();
        if (threadIdx.x == 0) {
            int n = 0;
#pragma unroll
            for (int w = 0; w < FR_WAVES; ++w) n += s_cnt[w];
            cnt[tile] = n;
        }
    }
}

// base [tiles]: the first row of every tile. score [rows][m], ext_c [rows]: the compacted scratch state.
template <int KIND, class T>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_fill(FrTrack tk, const unsigned *__restrict__ excl, RkRule rule, RkGraph g, double min_score,
                                                      int tile_rows, const int *__restrict__ cnt, const long long *__restrict__ base,
                                                      double *__restrict__ score, int *__restrict__ ext_c) {
    __shared__ double s_p[FR_STAGE * FR_LDS_ROW];
    __shared__ double s_f[FR_STAGE];
    __shared__ unsigned s_x[FR_STAGE];
    __shared__ int s_dst[FR_STAGE]; // the place of a staged row inside its tile (-1: dropped)
    __shared__ int s_cnt[FR_WAVES];
    const int ls = tk.gw + 1, m = tk.m, stage = fr_stage_rows(tile_rows);
    const long long tiles = fr_tiles(tk.V, tile_rows);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (cnt[tile] == 0) continue; // (the same in every thread of the workgroup)
        const long long t0 = fr_tile_first(tile, tile_rows), t1 = t0 + fr_tile_count(tile, tk.V, tile_rows), row0 = base[tile];
        int before = 0; // kept ids of the tile's earlier stages
        for (long long e0 = t0; e0 < t1; e0 += stage) {
            const int n = (int)min((long long)stage, t1 - e0);
            __syncthreads(); // (the previous stage is written out)
            fr_stage<KIND, T>(tk, excl, rule, g, e0, n, s_p, s_f, s_x);
            __syncthreads();
            const bool keep = (int)threadIdx.x < n && fr_keeps<KIND>(s_p, s_f, s_x, ls, m, threadIdx.x, min_score);
            const uint64_t b = __ballot(keep);
            if (lane_id() == 0) s_cnt[wave_id()] = __popcll(b);
            __syncthreads();
            int at = before + mbcnt(b), all = 0;
#pragma unroll
            for (int w = 0; w < FR_WAVES; ++w) {
                at += w < wave_id() ? s_cnt[w] : 0;
                all += s_cnt[w];
            }
            s_dst[threadIdx.x] = keep ? at : -1;
            if (keep) ext_c[row0 + at] = (int)(e0 + threadIdx.x);
            before += all;
            __syncthreads();
            for (int o = threadIdx.x; o < n * m; o += FR_BLOCK) {
                const int rl = o / m, c = o % m, d = s_dst[rl];
                if (d >= 0) score[(size_t)(row0 + d) * m + c] = rk_score<KIND>(s_p[rl * ls + c], s_f[rl], (s_x[rl] >> c) & 1u);
            }
        }
    }
}

// ---- the score at n_ids external ids: one thread per (id, column); out [n_ids][m] -------------------------------------------
template <int KIND, class T>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_score_at(FrTrack tk, const int *__restrict__ ids, int n_ids, const unsigned *__restrict__ excl,
                                                          RkRule rule, RkGraph g, double *__restrict__ out) {
    const int64_t total = (int64_t)n_ids * tk.m;
    for (int64_t t = (int64_t)blockIdx.x * FR_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * FR_BLOCK) {
        const int i = (int)(t / tk.m), col = (int)(t % tk.m);
        const int ext = ids[i];
        const unsigned x = excl ? excl[ext] : 0u;
        const bool gone = rk_masked_out(rule, ext) || ((x >> col) & 1u);
        out[t] = rk_score<KIND>(tk.p[(size_t)ext * tk.gw + col], rk_factor<KIND, T>(rule, g, ext, tk.ext2int[ext]), gone);
    }
}

// ---- the leaves of a sample: k_sm_leaves over the plane by external id -----------------------------------------------------
// leaves [m][t.Vt], nodes [m][t.node_stride], low [m][t.Vt] or NULL
template <int KIND, class T>
__global__ __launch_bounds__(SM_BLOCK) void k_fr_leaves(FrTrack tk, const unsigned *__restrict__ excl, RkRule rule, RkGraph g, double min_score, SmTree t,
                                                        double *__restrict__ leaves, double *__restrict__ nodes, double *__restrict__ low,
                                                        int *__restrict__ support) {
    constexpr int ROW_A = SM_SUB + 1, ROW_B = SM_SUB / 2;
    __shared__ double s_a[Q_LANES * ROW_A];
    __shared__ double s_b[Q_LANES * ROW_B];
    __shared__ double s_n8[Q_LANES * 8];
    __shared__ double s_f[SM_SUB];
    __shared__ unsigned s_x[SM_SUB];
    __shared__ unsigned s_cnt[Q_LANES];
    const int tile = blockIdx.x, n = tk.m;
    if (threadIdx.x < Q_LANES) s_cnt[threadIdx.x] = 0u;
    for (int sb = 0; sb < SM_TILE / SM_SUB; ++sb) {
        const long long base = (long long)tile * SM_TILE + (long long)sb * SM_SUB;
        __syncthreads(); // (the previous subtile's levels are out)
        {
            const long long ext = base + threadIdx.x;
            unsigned x = 0xffffffffu; // (an id beyond V weighs nothing)
            double f = 0.0;
            if (ext < (long long)tk.V) {
                x = excl ? excl[ext] : 0u;
                if (rk_masked_out(rule, (int)ext)) x = 0xffffffffu;
                f = rk_factor<KIND, T>(rule, g, (int)ext, tk.ext2int[ext]);
            }
            s_x[threadIdx.x] = x;
            s_f[threadIdx.x] = f;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < SM_SUB * n; o += SM_BLOCK) { // (consecutive threads read consecutive doubles of a row)
            const int id = o / n, lane = o % n;
            const long long ext = base + id;
            const double v = ext < (long long)tk.V ? tk.p[(size_t)ext * tk.gw + lane] : 0.0;
            s_a[lane * ROW_A + id] = sample_weight(rk_score<KIND>(v, s_f[id], (s_x[id] >> lane) & 1u), min_score);
        }
        __syncthreads();
        sm_subtile_out(s_a, s_b, s_n8, s_cnt, n, t, base, sb, leaves, low);
    }
    __syncthreads();
    sm_tile_nodes(s_n8, s_cnt, n, t, tile, nodes, support);
}

} // namespace dppr
