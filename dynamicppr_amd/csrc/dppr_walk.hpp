// dppr_walk.hpp -- forward random walks over an epoch's out-CSR (dppr_walks) and the fold of the residuals at their endpoints
// (dppr_refine_at / dppr_group_refine_at). Never called from the update path.
//
// THE WALK is walk_step of dppr_walk_plan.hpp, the one definition the host restatement runs too: Philox4x32-10 keyed by the seed,
// counter (w, v, t, 0); stop below floor(0.15 * 2^32); one of outdeg + 1 choices by __umul64hi, the last of them death. A step
// is ten Philox rounds (20 v_mul_hi_u32 / v_mul_lo_u32 pairs) and TWO DEPENDENT RANDOM LOADS: out_row_ptr[u] and [u + 1] (two
// adjacent ints, one line), then out_col[rs + j]. What a wave waits for is latency, and the only thing that hides it is other waves: the
// kernels keep their registers low enough for eight waves per SIMD.
//
// k_walk<true>, LANE REFILL. Walk lengths are geometric (mean 1 / 0.15 = 6.7 draws, the longest of 64 about 30): one walk per
// thread leaves a wave mostly idle behind its longest lane. A wave owns the contiguous range walk_range(total, wave) of the index
// space q * W + w. Every round the idle lanes are counted (ballot), an idle lane takes index next + (idle lanes below it) (mbcnt)
// if that is still inside the range, `next` -- wave-uniform, a scalar -- advances by the count; then every busy lane takes one
// step, and a lane whose walk ended stores the endpoint AT THE WALK'S OWN INDEX and is idle again. The wave leaves when the range
// is empty and every lane is idle. No atomics, no LDS: which lane ran a walk changes nothing, the walk is a function of its index.
// k_walk<false>, ONE WALK PER THREAD: thread i runs walk i to its end. The same bits; kept for the measurement and for one test
// (dppr_debug_walk_form).
// Endpoint: the external id of the vertex the walk stopped on (int2ext; the start's own id where it has no internal id), -1 for
// a walk that died.
//
// k_walk_fold: the fold of include/dppr.h over the W slots of every query, for S = fold(t) and sumsq = fold(t * t) in one pass,
// t_w = r_i[endpoint w] (+0.0 for a dead walk or a vertex without a row): the sparse pass of dppr_dot.hpp with weight 1.0 (1.0 * t
// is t), id -1 a +0.0 term instead of a rejection, and the staged rows squared in place (__dmul_rn) for the second fold. The
// pieces -- dot_subtile, DotCarry, the tile table, k_dot_combine over 2 n "lanes" -- are those of the dot products.
// k_refine_finish: corr = S / W (one __ddiv_rn), est = p + corr (one __dadd_rn).
// Every store is an ordinary vector store.
#pragma once

#include "dppr_common.hpp"
#include "dppr_dot.hpp"
#include "dppr_walk_plan.hpp"

namespace dppr {

static_assert(WALK_WAVE == WAVE && WALK_BLOCK == BLOCK, "dppr_walk_plan.hpp restates the wave and the workgroup");

__device__ __forceinline__ int walk_endpoint(const int *__restrict__ int2ext, int u, int v) { return u >= 0 ? int2ext[u] : v; }

// starts [m] external ids (checked by the host: inside [0, V)); ends [total]; total = m * W <= 2^26
template <bool REFILL>
__global__ __launch_bounds__(WALK_BLOCK) void k_walk(const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                     const int *__restrict__ ext2int, const int *__restrict__ int2ext,
                                                     const int *__restrict__ starts, unsigned W, long long total, long long per_wave,
                                                     unsigned k0, unsigned k1, int *__restrict__ ends) {
    if constexpr (!REFILL) {
        const long long idx = (long long)blockIdx.x * WALK_BLOCK + threadIdx.x;
        if (idx >= total) return;
        const unsigned q = (unsigned)idx / W, w = (unsigned)idx - q * W;
        const int v = starts[q];
        int u = ext2int[v], end = WALK_DIED;
        for (int t = 0; t < WALK_MAX_STEPS; ++t) {
            const int nx = walk_step(row_ptr, col, u, (unsigned)v, w, (unsigned)t, k0, k1);
            if (nx == WALK_STOPPED) {
                end = walk_endpoint(int2ext, u, v);
                break;
            }
            if (nx == WALK_DIED) break;
            u = nx;
        }
        ends[idx] = end;
    } else {
        int64_t lo, hi;
        walk_range(total, per_wave, (int64_t)blockIdx.x * WALK_WAVES_PER_BLOCK + wave_id(), &lo, &hi);
        int64_t next = lo; // (the same in every lane)
        int idx = -1;        // the walk this lane runs; -1: idle
        int u = -1, v = 0, t = 0;
        unsigned w = 0;
        for (;;) {
            const uint64_t idle = __ballot(idx < 0);
            if (idle && next < hi) {
                const int64_t cand = next + mbcnt(idle);
                if (idx < 0 && cand < hi) {
                    idx = (int)cand;
                    const unsigned q = (unsigned)idx / W;
                    w = (unsigned)idx - q * W;
                    v = starts[q];
                    u = ext2int[v];
                    t = 0;
                }
                next = next + (int64_t)__popcll(idle) < hi ? next + (int64_t)__popcll(idle) : hi;
            }
            if (__ballot(idx >= 0) == 0) break; // (the range is empty and every lane is idle)
            if (idx >= 0) {
                const int nx = walk_step(row_ptr, col, u, (unsigned)v, w, (unsigned)t, k0, k1);
                int end = WALK_DIED;
                bool over = true;
                if (nx == WALK_STOPPED)
                    end = walk_endpoint(int2ext, u, v);
                else if (nx >= 0 && ++t < WALK_MAX_STEPS)
                    over = false;
                if (over) {
                    ends[idx] = end;
                    idx = -1;
                } else {
                    u = nx;
                }
            }
        }
    }
}

// S and sumsq of every query: x = r of the state (rows of gw doubles, n lanes in use), ends [m][W] external ids or -1, the tile
// table of m queries of W slots. part[i * stride + col] (S of lane i) and part[(n + i) * stride + col] (sumsq).
__global__ __launch_bounds__(DOT_TILE) void k_walk_fold(const double *__restrict__ x, int gw, int n, const int *__restrict__ ext2int,
                                                        const int *__restrict__ ends, const DotTile *__restrict__ tiles,
                                                        long long n_tiles, double *__restrict__ part, long long stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dot_lds[];
    const int ls = gw + 1, tid = (int)threadIdx.x;
    double *s_x = reinterpret_cast<double *>(dot_lds);
    double *s_h = s_x + DOT_TILE * ls;
    double *s_part = s_h + DOT_HS;
    const int G = dot_groups_dev(n);
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const DotTile tl = tiles[t];
        DotCarry carry, carry2;
        double sum = 0.0, sum2 = 0.0;
        for (int sub = 0; sub < DOT_SUB; ++sub) {
            const int cnt = min(DOT_TILE, tl.cnt - sub * DOT_TILE);
            double v = 0.0, v2 = 0.0; // (a subtile of padding)
            if (cnt > 0) {
                __syncthreads(); // (the fold of the previous subtile is over)
                int row = -1;
                if (tid < cnt) {
                    const int id = ends[tl.e0 + (long long)sub * DOT_TILE + tid];
                    if (id >= 0) row = ext2int[id]; // (an endpoint is an id the walk kernel wrote: -1 or inside [0, V))
                }
                s_h[tid] = 1.0;
                double *dst = s_x + tid * ls;
                for (int l = 0; l < gw; ++l) dst[l] = row >= 0 ? x[(size_t)row * gw + l] : 0.0;
                __syncthreads();
                v = dot_subtile(s_h, s_x, s_part, ls, n, n, G);
                __syncthreads();
                for (int l = 0; l < gw; ++l) dst[l] = __dmul_rn(dst[l], dst[l]);
                __syncthreads();
                v2 = dot_subtile(s_h, s_x, s_part, ls, n, n, G);
            }
            sum = carry.push(sub, v);
            sum2 = carry2.push(sub, v2);
        }
        if (tid < n) {
            part[(size_t)tid * (size_t)stride + (size_t)tl.col] = sum;
            part[(size_t)(n + tid) * (size_t)stride + (size_t)tl.col] = sum2;
        }
    }
}

// folded [m][2 n] (S of every lane, then sumsq of every lane); res: est [m][n] | corr [m][n] | sumsq [m][n]
__global__ __launch_bounds__(BLOCK) void k_refine_finish(const double *__restrict__ p, int gw, int n, const int *__restrict__ ext2int,
                                                         const int *__restrict__ ids, int m, int W, const double *__restrict__ folded,
                                                         double *__restrict__ res) {
    const int mn = m * n;
    for (int j = blockIdx.x * BLOCK + threadIdx.x; j < mn; j += gridDim.x * BLOCK) {
        const int q = j / n, i = j % n, row = ext2int[ids[q]];
        const double pv = row >= 0 ? p[(size_t)row * gw + i] : 0.0;
        const double corr = __ddiv_rn(folded[(size_t)q * 2 * n + i], (double)W);
        res[j] = __dadd_rn(pv, corr);
        res[mn + j] = corr;
        res[2 * mn + j] = folded[(size_t)q * 2 * n + n + i];
    }
}

} // namespace dppr
