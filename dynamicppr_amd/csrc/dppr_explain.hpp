// dppr_explain.hpp -- explain a score (dppr_explain_at / dppr_group_explain_at): the top contributing out-edges of given vertices
// and the path of largest contributions towards a lane's seeds. Never called from the update path.
//
// CONTRIBUTION (include/dppr.h). For lane i, a vertex u of stored out-degree d and a DISTINCT head w stored mult times:
//     c_i(u, w) = (((1.0 - 0.15) * p_i[w]) * (double)mult) / (double)(d + 1)
// two explicit round-to-nearest multiplies and one divide (ex_contribution: the compiler never contracts or reorders them). The
// contributor order of (u, i) is the heads with c > 0, c descending, external id ascending.
//
// ROWS. An out-row is stored sorted by internal head id (dppr_builder.hpp: key src << bits | dst), so the copies of a head are
// adjacent: an entry STARTS A RUN iff it is the row's first or its predecessor in the row differs -- whether or not the
// predecessor belongs to the same step of the wave -- and the run ends at the next start: a bit of the step's ballot of starts,
// or, for the one run that reaches the step's end, the upper bound of the head in the sorted rest of the row (one look at the next
// entry first; a binary search only if the run does go on). Only the lane that holds the start forms c. The first form of this
// walk searched the upper bound for EVERY start: some ten dependent loads per step, and the wave of the longest row on any path
// was the call (profiles/explain_times.md). ex_row_best is the one walk both kernels share: a wave
// takes `step` entries at a time (64; dppr_debug_explain lowers it, so that a test drives a run across every step boundary),
// every lane keeps the best head it has seen that stands STRICTLY AFTER (prev_c, prev_ext) in the contributor order, and a
// butterfly over the wave leaves the arg-max in every lane. No LDS, no atomic, no scratch memory.
//
// SHAPE. One wave per (query, lane) in both kernels: the choice over one wave per query serving all lanes, because the waves of a
// query then need no common loop over n lanes of live registers, a lane's f rounds stop at that lane's own count, and the rows of
// the m queried vertices are short (the second and later readers of a row find it in L2).
//   k_ex_first   f rounds of ex_row_best, each strictly after the previous winner, write nbr / nbr_mult / nbr_c in contributor
//                order with ordinary vector stores by lane 0, the tails by the wave; self; deg and distinct by the wave of lane 0.
//   k_ex_path    the wave loops the hops itself: the seed test, the arg-max over the current vertex's row, the on-path test, the
//                append. Lane t of the wave holds path[t] (internal id); the on-path test is one ballot. No other wave is ever
//                waited for.
// MEMO (dppr_explain_plan.hpp). The paths of a lane end in the same few vertices near its seeds, so k_ex_path may share its
// arg-maxes through a table of one 64-bit word (next internal id, mult) per (live row, lane): one relaxed agent-scope atomic load;
// on EX_MEMO_UNKNOWN the wave computes the arg-max and stores it with one relaxed atomic store. An entry only ever goes from
// unknown to the one value that is a function of the state and the epoch, so a lost or stale read costs a recomputation, never a
// different result; c is always recomputed from p, mult and d.
// DESIGN.md section 9n has the figures of this shape.
#pragma once

#include "dppr_common.hpp"
#include "dppr_explain_plan.hpp"
#include "dppr_rank.hpp"

namespace dppr {

static_assert(EX_BLOCK == 4 * WAVE && EX_WAVE_ROWS == WAVE && Q_LANES == GS_MAX, "dppr_explain_plan.hpp restates the wave and the lanes");
static_assert(DPPR_EXPLAIN_MAX_DEPTH <= WAVE, "lane t of a wave holds path[t] for every t a vertex is compared with");

struct ExIn {              // what both kernels read
    const double *p;       // the state: rows of gw doubles by internal id
    int gw, n;
    const int *ext2int, *int2ext;
    const int *ids;        // [m] external
    int m;
    RkGraph g;             // the epoch's out-CSR and the live zone
    RkLanes l;             // the seeds of the lanes
};

struct ExFirstOut {        // NULL: not asked for
    int *deg, *distinct;   // [m]
    double *self;          // [m][n]
    int *nbr_count;        // [m][n]
    int *nbr, *nbr_mult;   // [m][n][f]
    double *nbr_c;
};
struct ExPathOut {         // NULL: not asked for
    int *len, *end;        // [m][n]
    int *path;             // [m][n][depth + 1]
    double *path_p;
    double *path_c;        // [m][n][depth]
};

struct ExBest { // wave-uniform; c == 0.0: the order holds nothing (more)
    double c;
    int ext, w, mult;
};

__device__ __forceinline__ double ex_contribution(double pw, int mult, double den) {
    return __ddiv_rn(__dmul_rn(__dmul_rn(ONE_MINUS_ALPHA, pw), (double)mult), den);
}
// (ca, ea) strictly before (cb, eb) in the contributor order
__device__ __forceinline__ bool ex_before(double ca, int ea, double cb, int eb) { return ca > cb || (ca == cb && ea < eb); }

// h of lane i at internal id u (u < 0: no id)
__device__ __forceinline__ double ex_h(const RkLanes &l, int i, int u) {
    if (u < 0) return 0.0;
    const int s = l.src.s[i];
    if (s >= 0) return u == s ? 1.0 : 0.0;
    if (l.seeds.off[i + 1] == l.seeds.off[i]) return 0.0; // (a lane without seeds: the table is never read)
    return tg_h(l.tg, i, u);
}

__device__ __forceinline__ double ex_uniform(double x) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}

// distinct heads of row [r0, r1) (wave-uniform bounds and result)
__device__ __forceinline__ int ex_row_distinct(const RkGraph &g, int r0, int r1, int step) {
    int cnt = 0;
    for (int e0 = r0; e0 < r1; e0 += step) {
        const int e = e0 + lane_id();
        bool first = false;
        if (lane_id() < step && e < r1) first = e == r0 || g.out_col[e - 1] != g.out_col[e];
        cnt += __popcll(__ballot(first));
    }
    return cnt;
}

// The first head of row [r0, r1) (wave-uniform, r0 < r1 or the row is empty) in lane i's contributor order that stands strictly
// after (prev_c, prev_ext); prev_c = +inf, prev_ext = -1: the first of all.
__device__ __forceinline__ ExBest ex_row_best(const ExIn &in, int i, int r0, int r1, int step, double prev_c, int prev_ext) {
    const RkGraph &g = in.g;
    const double den = (double)(r1 - r0 + 1);
    double bc = 0.0;
    int bext = 0x7fffffff, bw = -1, bm = 0;
    for (int e0 = r0; e0 < r1; e0 += step) {
        const int e = e0 + lane_id();
        const int e_end = min(e0 + step, r1); // (wave-uniform) one past the step's last entry
        int w = -1, before = -1;
        if (e < e_end) {
            w = g.out_col[e]; // (a plain load, not ld_stream: the row is read again by every later round and hop, from L2)
            if (e != r0) before = g.out_col[e - 1];
        }
        const bool first = e < e_end && (e == r0 || before != w);
        const unsigned long long starts = __ballot(first); // the runs that start in this step
        if (first && (unsigned)w < (unsigned)g.n_int) {     // (inside a run: its start forms c; a head of a stored edge is live: always)
            // the end of the run: the next start of the step; a run that reaches the step's end goes on while the row holds w -- one
            // look at the next entry, and only behind it the upper bound of w in the sorted rest of the row
            const unsigned long long later = lane_id() < WAVE - 1 ? starts >> (lane_id() + 1) : 0ull;
            int run_end = e_end;
            if (later) {
                run_end = e + __ffsll((long long)later);
            } else if (e_end < r1 && g.out_col[e_end] == w) {
                int lo = e_end + 1, hi = r1;
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (g.out_col[mid] <= w) lo = mid + 1;
                    else hi = mid;
                }
                run_end = lo;
            }
            const int mult = run_end - e;
            const double c = ex_contribution(in.p[(size_t)w * in.gw + i], mult, den);
            const int ext = in.int2ext[w];
            if (c > 0.0 && ex_before(prev_c, prev_ext, c, ext) && ex_before(c, ext, bc, bext)) { // (c > 0: false for a NaN)
                bc = c;
                bext = ext;
                bw = w;
                bm = mult;
            }
        }
    }
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) {
        const double oc = __shfl_xor(bc, off, WAVE);
        const int oext = __shfl_xor(bext, off, WAVE), ow = __shfl_xor(bw, off, WAVE), om = __shfl_xor(bm, off, WAVE);
        if (ex_before(oc, oext, bc, bext)) {
            bc = oc;
            bext = oext;
            bw = ow;
            bm = om;
        }
    }
    ExBest b;
    b.c = ex_uniform(bc);
    b.ext = __builtin_amdgcn_readfirstlane(bext);
    b.w = __builtin_amdgcn_readfirstlane(bw);
    b.mult = __builtin_amdgcn_readfirstlane(bm);
    return b;
}

// grid: ex_grid(m, n), one wave per (query, lane)
__global__ __launch_bounds__(EX_BLOCK) void k_ex_first(ExIn in, int f, int step, ExFirstOut o) {
    const int pair = blockIdx.x * EX_PAIR_WAVES + wave_id();
    if (pair >= in.m * in.n) return;
    const int j = pair / in.n, i = pair - j * in.n;
    const int u = __builtin_amdgcn_readfirstlane(in.ext2int[in.ids[j]]);
    int r0 = 0, r1 = 0;
    if ((unsigned)u < (unsigned)in.g.n_int) { // (no id, parked: no row in the epoch)
        r0 = __builtin_amdgcn_readfirstlane(in.g.out_row_ptr[u]);
        r1 = __builtin_amdgcn_readfirstlane(in.g.out_row_ptr[u + 1]);
    }
    if (i == 0 && (o.deg || o.distinct)) {
        const int distinct = o.distinct ? ex_row_distinct(in.g, r0, r1, step) : 0;
        if (lane_id() == 0) {
            if (o.deg) o.deg[j] = r1 - r0;
            if (o.distinct) o.distinct[j] = distinct;
        }
    }
    if (o.self && lane_id() == 0) o.self[pair] = __dmul_rn(ALPHA, ex_h(in.l, i, u));
    if (!o.nbr_count && !o.nbr && !o.nbr_mult && !o.nbr_c) return;
    const size_t base = (size_t)pair * (size_t)f;
    double prev_c = __builtin_huge_val();
    int prev_ext = -1, cnt = 0;
    while (cnt < f) {
        const ExBest b = ex_row_best(in, i, r0, r1, step, prev_c, prev_ext);
        if (!(b.c > 0.0)) break;
        if (lane_id() == 0) {
            if (o.nbr) o.nbr[base + cnt] = b.ext;
            if (o.nbr_mult) o.nbr_mult[base + cnt] = b.mult;
            if (o.nbr_c) o.nbr_c[base + cnt] = b.c;
        }
        prev_c = b.c;
        prev_ext = b.ext;
        ++cnt;
    }
    for (int k = cnt + lane_id(); k < f; k += WAVE) {
        if (o.nbr) o.nbr[base + k] = -1;
        if (o.nbr_mult) o.nbr_mult[base + k] = 0;
        if (o.nbr_c) o.nbr_c[base + k] = 0.0;
    }
    if (o.nbr_count && lane_id() == 0) o.nbr_count[pair] = cnt;
}

// grid: ex_grid(m, n), one wave per (query, lane). memo: [live rows][n] words or NULL (every arg-max is computed)
__global__ __launch_bounds__(EX_BLOCK) void k_ex_path(ExIn in, int depth, int step, unsigned long long *__restrict__ memo, ExPathOut o) {
    const int pair = blockIdx.x * EX_PAIR_WAVES + wave_id();
    if (pair >= in.m * in.n) return;
    const int j = pair / in.n, i = pair - j * in.n;
    const size_t base_v = (size_t)pair * ((size_t)depth + 1), base_c = (size_t)pair * (size_t)depth;
    int cur_ext = __builtin_amdgcn_readfirstlane(in.ids[j]);
    int cur = __builtin_amdgcn_readfirstlane(in.ext2int[cur_ext]);
    int mine = -2; // lane t: the internal id of path[t] (-2: none yet; -1: a vertex without an id)
    int t = 0, end = DPPR_EXPLAIN_END_DEPTH;
    for (;;) {
        if (lane_id() == 0) {
            if (o.path) o.path[base_v + t] = cur_ext;
            if (o.path_p) o.path_p[base_v + t] = cur >= 0 ? in.p[(size_t)cur * in.gw + i] : 0.0;
        }
        if (lane_id() == t) mine = cur;
        if (ex_h(in.l, i, cur) > 0.0) {
            end = DPPR_EXPLAIN_END_SEED;
            break;
        }
        if (t == depth) {
            end = DPPR_EXPLAIN_END_DEPTH;
            break;
        }
        ExBest b;
        b.c = 0.0;
        b.ext = b.w = -1;
        b.mult = 0;
        if ((unsigned)cur < (unsigned)in.g.n_int) {
            const int r0 = __builtin_amdgcn_readfirstlane(in.g.out_row_ptr[cur]), r1 = __builtin_amdgcn_readfirstlane(in.g.out_row_ptr[cur + 1]);
            unsigned long long word = EX_MEMO_UNKNOWN;
            unsigned long long *slot = memo ? memo + (size_t)cur * in.n + i : nullptr;
            if (slot) {
                word = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                word = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(word >> 32)) << 32) |
                       (unsigned)__builtin_amdgcn_readfirstlane((int)(word & 0xffffffffull));
            }
            if (word == EX_MEMO_UNKNOWN) {
                b = ex_row_best(in, i, r0, r1, step, __builtin_huge_val(), -1);
                if (slot && lane_id() == 0)
                    __hip_atomic_store(slot, ((unsigned long long)(unsigned)b.w << 32) | (unsigned)b.mult, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                const int w = (int)(word >> 32);
                if ((unsigned)w < (unsigned)in.g.n_int) { // (-1: the order of this pair is empty)
                    b.w = w;
                    b.mult = (int)(word & 0xffffffffull);
                    b.ext = __builtin_amdgcn_readfirstlane(in.int2ext[w]);
                    b.c = ex_uniform(ex_contribution(in.p[(size_t)w * in.gw + i], b.mult, (double)(r1 - r0 + 1)));
                }
            }
        }
        if (!(b.c > 0.0)) {
            end = DPPR_EXPLAIN_END_DEAD;
            break;
        }
        if (__ballot(mine == b.w)) {
            end = DPPR_EXPLAIN_END_CYCLE;
            break;
        }
        if (o.path_c && lane_id() == 0) o.path_c[base_c + t] = b.c;
        cur = b.w;
        cur_ext = b.ext;
        ++t;
    }
    const int len = t + 1;
    for (int k = len + lane_id(); k <= depth; k += WAVE) {
        if (o.path) o.path[base_v + k] = -1;
        if (o.path_p) o.path_p[base_v + k] = 0.0;
    }
    if (o.path_c)
        for (int k = len - 1 + lane_id(); k < depth; k += WAVE) o.path_c[base_c + k] = 0.0;
    if (lane_id() == 0) {
        if (o.len) o.len[pair] = len;
        if (o.end) o.end[pair] = end;
    }
}

} // namespace dppr
