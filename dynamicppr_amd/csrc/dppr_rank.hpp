// dppr_rank.hpp -- ranked candidates (dppr_topk_ranked / dppr_group_topk_ranked / dppr_rank_score_at / dppr_group_rank_score_at):
// a per-vertex factor, a candidate mask and a per-lane exclusion of the seeds and their neighbours, applied between the state and
// the selection. Never called from the update path.
//
// SCORE (include/dppr.h). For lane i and a row of the state with p = p_i[v]:
//     NONE: p      DEV: p * g[ext(v)]      DEG: p * (double)(outdeg(v) + 1)      INV_DEG: p / (double)(outdeg(v) + 1)
// one explicit round-to-nearest multiply or divide (rk_score: the compiler never contracts or reorders it); +0.0 where the vertex is
// masked out or excluded for the lane. rk_score is the one score function: k_rk_scores and k_rk_score_at share it.
//
// SHAPE: marked, then materialised.
//   k_rk_rowlen   one thread per seed of the call: the lengths of its out-row and its in-row, for the host's piece list
//                 (dppr_rank_plan.hpp: a row is cut into pieces of at most `piece` entries)
//   k_rk_mark     one wave per piece: the entries of the piece read coalesced, bit `lane` of excl[w] set by one 32-bit vector
//                 atomic OR per entry; the seeds' own bits by one thread per seed. excl is one word per LIVE row, zeroed per call
//                 (parked rows have no edges and are never seeds). Nothing else is written, and an OR does not depend on the order
//                 in which the pieces arrive.
//   k_rk_scores   one tile of dppr_topk.hpp (tk_stage_tile) per step; per row, beside the external id, the exclusion word (all
//                 ones where the mask takes the vertex out) and the factor -- a DEV factor gathered by external id, a degree
//                 from out_row_ptr by internal id -- then n scores per row into the COMPACTED scratch state
//                 score[c * n + lane] with ext_c[c].
//                 Templated on the factor kind and the dtype of g: the NONE path carries no gather.
//   selection     dppr_topk.hpp over the scratch as a state of n lanes without a parked zone, as it is.
//   k_rk_score_at one thread per (id, lane); the row, and with it the exclusion word and the degree, through ext2int.
// DESIGN.md section 9k has the byte counts of this shape.
#pragma once

#include "dppr_common.hpp"
#include "dppr_multi.hpp"
#include "dppr_rank_plan.hpp"
#include "dppr_targets.hpp"
#include "dppr_topk.hpp"

namespace dppr {

static_assert(RK_BLOCK == 4 * WAVE && Q_LANES == GS_MAX && Q_LANES == TG_LANES && TK_TILE_LDS_ROW == GS_MAX + 1,
              "dppr_rank_plan.hpp restates the wave and the lanes, dppr_topk.hpp the lanes");

// the seeds of a call's lanes: a source lane's from src, a set lane's from the group's seed table
struct RkLanes {
    SrcN src;
    TgDev tg;       // (never read when every lane is a source lane)
    RkSeeds seeds;  // where every lane's seeds lie in the flat list
};

struct RkGraph { // the epoch's two CSRs by internal id (NULL where the spec needs none), the live zone
    const int *out_row_ptr, *out_col;
    const int *in_row_ptr;
    const Adj *in_adj;
    int n_int, V;
};

struct RkRule { // what a vertex's own data decide: the mask and the factor
    const uint8_t *mask; // [V] by external id (NULL: no mask)
    int deny;            // 1: mask != 0 takes the vertex out, 0: mask == 0 does
    const void *g;       // [V] by external id (DEV)
};

__device__ __forceinline__ int rk_lane_of_pos(const RkLanes &l, int pos) {
    int lane = 0;
#pragma unroll
    for (int i = 1; i < GS_MAX; ++i) lane += pos >= l.seeds.off[i] ? 1 : 0; // (off is non-decreasing: the last lane that starts at or before pos)
    return lane;
}
__device__ __forceinline__ int rk_seed_at(const RkLanes &l, int lane, int pos) {
    const int s = l.src.s[lane];
    return s >= 0 ? s : l.tg.ids[l.tg.off[lane] + (pos - l.seeds.off[lane])];
}

// ---- the one score function ------------------------------------------------------------------------------------------------
template <int KIND> __device__ __forceinline__ double rk_score(double p, double f, bool out) {
    if (out) return 0.0;
    if (KIND == DPPR_FACTOR_NONE) return p;
    if (KIND == DPPR_FACTOR_INV_DEG) return __ddiv_rn(p, f);
    return __dmul_rn(p, f); // DEV, DEG
}
// ... and its factor at a vertex: ext its external id, row its internal id (< 0: none)
template <int KIND, class T> __device__ __forceinline__ double rk_factor(const RkRule &rule, const RkGraph &g, int ext, int row) {
    if (KIND == DPPR_FACTOR_DEV) return (double)static_cast<const T *>(rule.g)[ext];
    if (KIND == DPPR_FACTOR_DEG || KIND == DPPR_FACTOR_INV_DEG) {
        const int deg = (unsigned)row < (unsigned)g.n_int ? g.out_row_ptr[row + 1] - g.out_row_ptr[row] : 0; // (parked, no row: 0)
        return (double)(deg + 1);
    }
    return 0.0;
}
__device__ __forceinline__ bool rk_masked_out(const RkRule &rule, int ext) {
    if (!rule.mask) return false;
    return (rule.mask[ext] != 0) == (rule.deny != 0);
}

// ---- marking -------------------------------------------------------------------------------------------------------------
// len [total][2]: out-row, in-row
__global__ __launch_bounds__(RK_BLOCK) void k_rk_rowlen(RkLanes l, RkGraph g, int *__restrict__ len) {
    const int total = l.seeds.off[GS_MAX];
    for (int pos = blockIdx.x * RK_BLOCK + threadIdx.x; pos < total; pos += gridDim.x * RK_BLOCK) {
        const int u = rk_seed_at(l, rk_lane_of_pos(l, pos), pos);
        const bool ok = (unsigned)u < (unsigned)g.V;
        len[2 * (size_t)pos] = ok ? g.out_row_ptr[u + 1] - g.out_row_ptr[u] : 0;
        len[2 * (size_t)pos + 1] = ok ? g.in_row_ptr[u + 1] - g.in_row_ptr[u] : 0;
    }
}

// items: the piece list (cl_item: position | direction | chunk). excl [n_int], zeroed by the caller.
__global__ __launch_bounds__(RK_BLOCK) void k_rk_mark(RkLanes l, RkGraph g, unsigned flags, int piece,
                                                      const unsigned long long *__restrict__ items, unsigned n_items,
                                                      unsigned *__restrict__ excl) {
    for (unsigned t = blockIdx.x * RK_WAVES + wave_id(); t < n_items; t += gridDim.x * RK_WAVES) {
        const unsigned long long it = items[t];
        const int pos = (int)cl_item_pos(it), dir = (int)cl_item_dir(it);
        const int lane = __builtin_amdgcn_readfirstlane(rk_lane_of_pos(l, pos));
        const int u = __builtin_amdgcn_readfirstlane(rk_seed_at(l, lane, pos));
        if ((unsigned)u >= (unsigned)g.V) continue;
        const int *rp = dir ? g.in_row_ptr : g.out_row_ptr;
        const int r0 = __builtin_amdgcn_readfirstlane(rp[u]), r1 = __builtin_amdgcn_readfirstlane(rp[u + 1]);
        const long long lo = (long long)r0 + (long long)cl_item_chunk(it) * piece;
        const long long hi = min((long long)r1, lo + piece);
        const unsigned bit = 1u << lane;
        for (long long e = lo + lane_id(); e < hi; e += WAVE) {
            const int w = dir ? g.in_adj[e].v : ld_stream(g.out_col + e);
            if ((unsigned)w < (unsigned)g.n_int) atomicOr(&excl[w], bit);
        }
    }
    if (flags & DPPR_EXCLUDE_SEEDS) {
        const int total = l.seeds.off[GS_MAX];
        for (int pos = blockIdx.x * RK_BLOCK + threadIdx.x; pos < total; pos += gridDim.x * RK_BLOCK) {
            const int lane = rk_lane_of_pos(l, pos);
            const int u = rk_seed_at(l, lane, pos);
            if ((unsigned)u < (unsigned)g.n_int) atomicOr(&excl[u], 1u << lane);
        }
    }
}

// ---- the scratch state ---------------------------------------------------------------------------------------------------
// st: the state (rows of gw doubles; gw even for a group, 1 for a slot). excl: [n_int] or NULL (nothing is excluded).
// score: [st.rows][st.n], ext_c: [st.rows].
template <int KIND, class T>
__global__ __launch_bounds__(TK_TILE_BLOCK) void k_rk_scores(TkState st, const int *__restrict__ i2e, const unsigned *__restrict__ excl,
                                                             RkRule rule, RkGraph g, double *__restrict__ score, int *__restrict__ ext_c) {
    __shared__ double s_p[TK_TILE_ROWS * TK_TILE_LDS_ROW];
    __shared__ double s_f[TK_TILE_ROWS];
    __shared__ unsigned s_x[TK_TILE_ROWS];
    const int n = st.n, ls = st.gw + 1;
    const int n_tiles = (st.rows + TK_TILE_ROWS - 1) / TK_TILE_ROWS;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int c0 = tile * TK_TILE_ROWS, cnt = min(TK_TILE_ROWS, st.rows - c0);
        __syncthreads(); // (the scores of the previous tile are out)
        tk_stage_tile(st, i2e, c0, cnt, s_p, ext_c, [&](int rl, int row, int ext) {
            unsigned x = (excl && row < st.n_int) ? excl[row] : 0u;
            if (rk_masked_out(rule, ext)) x = 0xffffffffu;
            s_x[rl] = x;
            s_f[rl] = rk_factor<KIND, T>(rule, g, ext, row);
        });
        __syncthreads();
        for (int o = threadIdx.x; o < cnt * n; o += TK_TILE_BLOCK) {
            const int rl = o / n, lane = o % n;
            score[(size_t)c0 * n + o] = rk_score<KIND>(s_p[rl * ls + lane], s_f[rl], (s_x[rl] >> lane) & 1u);
        }
    }
}

// the score at m external ids: one thread per (id, lane); out [m][n]
template <int KIND, class T>
__global__ __launch_bounds__(RK_BLOCK) void k_rk_score_at(const double *__restrict__ p, int gw, int n, const int *__restrict__ ext2int,
                                                          const int *__restrict__ ids, int m, const unsigned *__restrict__ excl,
                                                          RkRule rule, RkGraph g, double *__restrict__ out) {
    const int64_t total = (int64_t)m * n;
    for (int64_t t = (int64_t)blockIdx.x * RK_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * RK_BLOCK) {
        const int i = (int)(t / n), lane = (int)(t % n);
        const int ext = ids[i], row = ext2int[ext];
        const double v = row >= 0 ? p[(size_t)row * gw + lane] : 0.0;
        const unsigned x = (excl && (unsigned)row < (unsigned)g.n_int) ? excl[row] : 0u;
        const bool gone = rk_masked_out(rule, ext) || ((x >> lane) & 1u);
        out[t] = rk_score<KIND>(v, rk_factor<KIND, T>(rule, g, ext, row), gone);
    }
}

} // namespace dppr
