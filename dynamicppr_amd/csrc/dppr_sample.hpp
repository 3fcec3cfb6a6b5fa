// dppr_sample.hpp -- vertices drawn in proportion to a lane's score (dppr_sample / dppr_group_sample): a balanced sum tree over
// the weights of every lane in EXTERNAL id order and a descent per draw. Never called from the update path. The definition --
// weight, tree, uniform, step -- is include/dppr.h's, and its functions are those of dppr_sample_plan.hpp (sample_weight,
// sample_u, sample_scale, sample_step, sample_status), which the host compiles too. The score is rk_score / rk_factor /
// rk_masked_out of dppr_rank.hpp, read the way k_rk_score_at reads it, so a drawn id's weight is dppr_rank_score_at's bit for bit.
//
// SHAPE (dppr_sample_plan.hpp has the arithmetic: SmTree).
//   k_sm_leaves  one workgroup per TILE of 2048 external ids, a SUBTILE of 256 ids at a time: a thread per id fetches the row
//                (ext2int), the exclusion word, the mask and the factor; then the rows of the state are read coalesced, (id, lane)
//                by (id, lane), into LDS [lane][id]; the weights leave lane-major, 2 KB contiguous per lane and subtile; the
//                subtile's levels 1 .. 8 are built in LDS, ping-pong between two arrays (written out only for the plain form),
//                and positive leaves are counted with integer adds. After 8 subtiles one thread per lane adds the levels 9 .. 11
//                and the nodes of levels 8 .. 11 are stored. One integer atomic per lane and tile for the support.
//   k_sm_upper   one workgroup per lane: the levels 12 .. top, level by level (a child beyond its level's count is +0.0), then
//                the root, the status and nothing else into the result block.
//   k_sm_draw    a wave owns 256 consecutive draws of the call's index space, 64 at a time: every lane runs Philox for its own
//                draw and descends the stored levels down to a subtile (the top levels stay in L2); then, draw by draw, the wave
//                takes the subtile and x of one lane (v_readlane: the turn is wave-uniform), loads the subtile's 256 leaves, four
//                per lane, rebuilds the levels 1 .. 8 -- two local adds, then six butterfly steps (a + b == b + a bit for bit, so
//                the order of a pair is free) -- and finishes the descent on values read from the lanes that hold them. Ids and
//                weights are kept by the lane whose draw it was and written coalesced: draw j of lane i lies at [i][j - first].
//   k_sm_draw_plain  dppr_debug_sample_form(1): one thread per draw, every level read from memory.
// No floating-point atomic anywhere: two calls return identical bits. DESIGN.md section 9q has the byte counts of this shape.
#pragma once

#include "dppr_common.hpp"
#include "dppr_rank.hpp"
#include "dppr_sample_plan.hpp"

namespace dppr {

static_assert(SM_BLOCK == 4 * WAVE && SM_SUB == 4 * WAVE && SM_SUB == SM_BLOCK && Q_LANES == GS_MAX, "dppr_sample_plan.hpp restates the wave and the lanes");

struct SmOut { // the head of the result block
    double *total;  // [16]
    int *support;   // [16], zeroed by the caller
    int *status;    // [16]
};

// One level of a subtile in LDS: dst[lane][j] = src[lane][2j] + src[lane][2j + 1] for j < cnt, every lane; the positive leaves
// counted where the source is level 0. lo: where the level goes in the array of the low levels (NULL: not stored).
template <bool COUNT>
__device__ __forceinline__ void sm_level(const double *src, int src_row, double *dst, int dst_row, int cnt, int n, unsigned *s_cnt,
                                         double *__restrict__ lo, long long lo_stride) {
    for (int it = threadIdx.x; it < n * cnt; it += SM_BLOCK) {
        const int lane = it / cnt, j = it % cnt;
        const double a = src[lane * src_row + 2 * j], b = src[lane * src_row + 2 * j + 1];
        const double y = __dadd_rn(a, b);
        dst[lane * dst_row + j] = y;
        if (lo) lo[(long long)lane * lo_stride + j] = y;
        if (COUNT) {
            const unsigned c = (a > 0.0 ? 1u : 0u) + (b > 0.0 ? 1u : 0u);
            if (c) atomicAdd(&s_cnt[lane], c);
        }
    }
}

// The weights of a subtile, in LDS [lane][id] (s_a), leave lane-major; the subtile's levels 1 .. 7 between the two arrays, level 8
// into the tile's eight (s_n8). Shared by k_sm_leaves and its sibling over a forward track (dppr_ftrack_rank.hpp: k_fr_leaves).
__device__ __forceinline__ void sm_subtile_out(double *s_a, double *s_b, double *s_n8, unsigned *s_cnt, int n, const SmTree &t, long long base, int sb,
                                               double *__restrict__ leaves, double *__restrict__ low) {
    constexpr int ROW_A = SM_SUB + 1, ROW_B = SM_SUB / 2;
    for (int o = threadIdx.x; o < SM_SUB * n; o += SM_BLOCK) {
        const int lane = o / SM_SUB, id = o % SM_SUB;
        leaves[(size_t)lane * (size_t)t.Vt + (size_t)base + id] = s_a[lane * ROW_A + id];
    }
    // levels 1 .. 7 between the two arrays, level 8 into the tile's eight
    sm_level<true>(s_a, ROW_A, s_b, ROW_B, 128, n, s_cnt, low ? low + sample_low_off(t.Vt, 1) + (base >> 1) : nullptr, t.Vt);
    __syncthreads();
    sm_level<false>(s_b, ROW_B, s_a, ROW_A, 64, n, s_cnt, low ? low + sample_low_off(t.Vt, 2) + (base >> 2) : nullptr, t.Vt);
    __syncthreads();
    sm_level<false>(s_a, ROW_A, s_b, ROW_B, 32, n, s_cnt, low ? low + sample_low_off(t.Vt, 3) + (base >> 3) : nullptr, t.Vt);
    __syncthreads();
    sm_level<false>(s_b, ROW_B, s_a, ROW_A, 16, n, s_cnt, low ? low + sample_low_off(t.Vt, 4) + (base >> 4) : nullptr, t.Vt);
    __syncthreads();
    sm_level<false>(s_a, ROW_A, s_b, ROW_B, 8, n, s_cnt, low ? low + sample_low_off(t.Vt, 5) + (base >> 5) : nullptr, t.Vt);
    __syncthreads();
    sm_level<false>(s_b, ROW_B, s_a, ROW_A, 4, n, s_cnt, low ? low + sample_low_off(t.Vt, 6) + (base >> 6) : nullptr, t.Vt);
    __syncthreads();
    sm_level<false>(s_a, ROW_A, s_b, ROW_B, 2, n, s_cnt, low ? low + sample_low_off(t.Vt, 7) + (base >> 7) : nullptr, t.Vt);
    __syncthreads();
    sm_level<false>(s_b, ROW_B, s_n8 + sb, 8, 1, n, s_cnt, nullptr, 0);
}

// ... after the eight subtiles of a tile: one thread per lane adds the levels 9 .. 11, the nodes of levels 8 .. 11 are stored and
// the lane's positive leaves join its support (one integer atomic per lane and tile). The caller has synchronised.
__device__ __forceinline__ void sm_tile_nodes(const double *s_n8, const unsigned *s_cnt, int n, const SmTree &t, int tile, double *__restrict__ nodes,
                                              int *__restrict__ support) {
    if (threadIdx.x < n) { // levels 8 .. 11 of this lane's tile
        const int lane = threadIdx.x;
        double *nd = nodes + (size_t)lane * t.node_stride;
        double y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            y[j] = s_n8[lane * 8 + j];
            nd[t.off[8] + (size_t)tile * 8 + j] = y[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y[j] = __dadd_rn(y[2 * j], y[2 * j + 1]);
            nd[t.off[9] + (size_t)tile * 4 + j] = y[j];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            y[j] = __dadd_rn(y[2 * j], y[2 * j + 1]);
            nd[t.off[10] + (size_t)tile * 2 + j] = y[j];
        }
        nd[t.off[11] + (size_t)tile] = __dadd_rn(y[0], y[1]);
        if (s_cnt[lane]) atomicAdd(&support[lane], (int)s_cnt[lane]);
    }
}

// p: the state, rows of gw doubles. leaves [n][t.Vt], nodes [n][t.node_stride], low [n][t.Vt] or NULL.
template <int KIND, class T>
__global__ __launch_bounds__(SM_BLOCK) void k_sm_leaves(const double *__restrict__ p, int gw, int n, const int *__restrict__ ext2int,
                                                        const unsigned *__restrict__ excl, RkRule rule, RkGraph g, double min_score, SmTree t,
                                                        double *__restrict__ leaves, double *__restrict__ nodes, double *__restrict__ low,
                                                        int *__restrict__ support) {
    constexpr int ROW_A = SM_SUB + 1, ROW_B = SM_SUB / 2;
    __shared__ double s_a[Q_LANES * ROW_A];
    __shared__ double s_b[Q_LANES * ROW_B];
    __shared__ double s_n8[Q_LANES * 8];
    __shared__ double s_f[SM_SUB];
    __shared__ int s_row[SM_SUB];
    __shared__ unsigned s_x[SM_SUB];
    __shared__ unsigned s_cnt[Q_LANES];
    const int tile = blockIdx.x;
    if (threadIdx.x < Q_LANES) s_cnt[threadIdx.x] = 0u;
    for (int sb = 0; sb < SM_TILE / SM_SUB; ++sb) {
        const long long base = (long long)tile * SM_TILE + (long long)sb * SM_SUB;
        __syncthreads(); // (the previous subtile's levels are out)
        {
            const long long ext = base + threadIdx.x;
            int row = -1;
            unsigned x = 0xffffffffu; // (an id beyond V weighs nothing)
            double f = 0.0;
            if (ext < (long long)g.V) {
                row = ext2int[ext];
                x = (excl && (unsigned)row < (unsigned)g.n_int) ? excl[row] : 0u;
                if (rk_masked_out(rule, (int)ext)) x = 0xffffffffu;
                f = rk_factor<KIND, T>(rule, g, (int)ext, row);
            }
            s_row[threadIdx.x] = row;
            s_x[threadIdx.x] = x;
            s_f[threadIdx.x] = f;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < SM_SUB * n; o += SM_BLOCK) { // (consecutive threads read consecutive doubles of a row)
            const int id = o / n, lane = o % n;
            const int row = s_row[id];
            const double v = row >= 0 ? p[(size_t)row * gw + lane] : 0.0;
            s_a[lane * ROW_A + id] = sample_weight(rk_score<KIND>(v, s_f[id], (s_x[id] >> lane) & 1u), min_score);
        }
        __syncthreads();
        sm_subtile_out(s_a, s_b, s_n8, s_cnt, n, t, base, sb, leaves, low);
    }
    __syncthreads();
    sm_tile_nodes(s_n8, s_cnt, n, t, tile, nodes, support);
}

// the levels above a tile, one workgroup per lane
__global__ __launch_bounds__(SM_BLOCK) void k_sm_upper(double *__restrict__ nodes, SmTree t, SmOut out) {
    const int lane = blockIdx.x;
    double *nd = nodes + (size_t)lane * t.node_stride;
    for (int l = SM_TILE_LEVEL + 1; l <= t.top; ++l) {
        const unsigned c = t.cnt[l], cp = t.cnt[l - 1];
        const double *src = nd + t.off[l - 1];
        for (unsigned j = threadIdx.x; j < c; j += SM_BLOCK) {
            const double a = src[2 * (size_t)j];
            const double b = 2 * j + 1 < cp ? src[2 * (size_t)j + 1] : 0.0;
            nd[t.off[l] + j] = __dadd_rn(a, b);
        }
        __threadfence_block();
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double root = nd[t.off[t.top]];
        out.total[lane] = root;
        out.status[lane] = sample_status(root);
    }
}

// the stored part of a descent: from the root down to the subtile; x is the draw's u * root
__device__ __forceinline__ unsigned sm_descend_stored(const double *__restrict__ nd, const SmTree &t, double &x) {
    unsigned k = 0;
    for (int l = t.top; l > SM_SUB_LEVEL; --l) {
        const double *c = nd + t.off[l - 1];
        const double L = c[2 * (size_t)k];
        const double R = 2 * k + 1 < t.cnt[l - 1] ? c[2 * (size_t)k + 1] : 0.0;
        k = 2 * k + (sample_step(x, L, R) ? 1u : 0u);
    }
    return k;
}

__device__ __forceinline__ double sm_readlane(double v, int lane) { // lane: wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double sm_xor_add(double v, int mask) { return __dadd_rn(v, __shfl_xor(v, mask, WAVE)); }

// total = n * S draws; out_ids [n][S], out_w [n][S] or NULL
__global__ __launch_bounds__(SM_BLOCK) void k_sm_draw(const double *__restrict__ leaves, const double *__restrict__ nodes, SmTree t,
                                                      const double *__restrict__ totals, const int *__restrict__ status, int64_t S, int64_t total,
                                                      uint64_t first, uint64_t seed, int *__restrict__ out_ids, double *__restrict__ out_w) {
    const int64_t wave = (int64_t)blockIdx.x * (SM_BLOCK / WAVE) + wave_id();
    const int64_t lo = wave * SM_DRAWS_PER_WAVE, hi = lo + SM_DRAWS_PER_WAVE < total ? lo + SM_DRAWS_PER_WAVE : total;
    for (int64_t b = lo; b < hi; b += WAVE) {
        const int64_t my = b + lane_id();
        int i = 0, ok = 0;
        unsigned sub = 0;
        double x = 0.0;
        if (my < hi) {
            i = (int)(my / S);
            const uint64_t j = first + (uint64_t)(my % S);
            ok = status[i] == DPPR_SAMPLE_OK ? 1 : 0;
            if (ok) {
                x = sample_scale(sample_u(j, (uint32_t)i, seed), totals[i]);
                sub = sm_descend_stored(nodes + (size_t)i * t.node_stride, t, x);
            }
        }
        int my_id = -1;
        double my_w = 0.0;
        const int turns = hi - b < WAVE ? (int)(hi - b) : WAVE;
        for (int s = 0; s < turns; ++s) {
            if (!__builtin_amdgcn_readlane(ok, s)) continue;
            const int si = __builtin_amdgcn_readlane(i, s);
            const unsigned ssub = (unsigned)__builtin_amdgcn_readlane((int)sub, s);
            double sx = sm_readlane(x, s);
            const double2 *lf = reinterpret_cast<const double2 *>(leaves + (size_t)si * (size_t)t.Vt + (size_t)ssub * SM_SUB) + 2 * lane_id();
            const double2 y01 = lf[0], y23 = lf[1];
            double c[9]; // c[l]: the node of level l this lane lies under (l >= 2)
            const double a01 = __dadd_rn(y01.x, y01.y), a23 = __dadd_rn(y23.x, y23.y);
            c[2] = __dadd_rn(a01, a23);
#pragma unroll
            for (int l = 3; l <= 8; ++l) c[l] = sm_xor_add(c[l - 1], 1 << (l - 3));
            unsigned k = 0;
#pragma unroll
            for (int l = 8; l >= 3; --l) { // node m of level l - 1 is held by lane m << (l - 3) (and its neighbours)
                const double L = sm_readlane(c[l - 1], (int)((2 * k) << (l - 3)));
                const double R = sm_readlane(c[l - 1], (int)((2 * k + 1) << (l - 3)));
                k = 2 * k + (sample_step(sx, L, R) ? 1u : 0u);
            }
            { // level 2 -> 1: lane k holds both children
                const double L = sm_readlane(a01, (int)k), R = sm_readlane(a23, (int)k);
                k = 2 * k + (sample_step(sx, L, R) ? 1u : 0u);
            }
            const int holder = (int)(k >> 1);
            const double L = (k & 1u) ? sm_readlane(y23.x, holder) : sm_readlane(y01.x, holder);
            const double R = (k & 1u) ? sm_readlane(y23.y, holder) : sm_readlane(y01.y, holder);
            const bool right = sample_step(sx, L, R);
            k = 2 * k + (right ? 1u : 0u);
            if (lane_id() == s) {
                my_id = (int)(ssub * SM_SUB + k);
                my_w = right ? R : L;
            }
        }
        if (my < hi) {
            out_ids[my] = my_id;
            if (out_w) out_w[my] = my_w;
        }
    }
}

// dppr_debug_sample_form(1): one thread per draw, every level from memory (low: the levels 1 .. 7)
__global__ __launch_bounds__(SM_BLOCK) void k_sm_draw_plain(const double *__restrict__ leaves, const double *__restrict__ nodes,
                                                            const double *__restrict__ low, SmTree t, const double *__restrict__ totals,
                                                            const int *__restrict__ status, int64_t S, int64_t total, uint64_t first, uint64_t seed,
                                                            int *__restrict__ out_ids, double *__restrict__ out_w) {
    const int64_t my = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (my >= total) return;
    const int i = (int)(my / S);
    const uint64_t j = first + (uint64_t)(my % S);
    int id = -1;
    double w = 0.0;
    if (status[i] == DPPR_SAMPLE_OK) {
        double x = sample_scale(sample_u(j, (uint32_t)i, seed), totals[i]);
        size_t k = sm_descend_stored(nodes + (size_t)i * t.node_stride, t, x);
        const double *lw = low + (size_t)i * (size_t)t.Vt, *lf = leaves + (size_t)i * (size_t)t.Vt;
        for (int l = SM_SUB_LEVEL; l >= 1; --l) {
            const double *c = l > 1 ? lw + sample_low_off(t.Vt, l - 1) : lf;
            const double L = c[2 * k], R = c[2 * k + 1];
            k = 2 * k + (sample_step(x, L, R) ? 1 : 0);
        }
        id = (int)k;
        w = lf[k];
    }
    out_ids[my] = id;
    if (out_w) out_w[my] = w;
}

} // namespace dppr
