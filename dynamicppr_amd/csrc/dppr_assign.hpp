// dppr_assign.hpp -- the query that reduces over the LANE axis (dppr_assign / dppr_assign_at): every external id gets the class
// of its largest score over the lanes of up to 16 groups, the margin to the runner-up, the per-class counts and the flips
// against a previous labelling. Never called from the update path.
//
// The kernels walk the EXTERNAL ids in tiles of AS_TILE, so id order is the order of the threads and no output position comes
// from an atomic:
//   k_as_label<TEAM>  A vertex is read by a TEAM of 1, 2, 4 or 8 neighbouring lanes (as_team: the widest row of the call in one
//               step of 16-byte loads; a 128-byte row is one instruction of 8 lanes, a wave reads 8 whole rows at a time). The
//               tile's rows come from ext2int in one coalesced read into LDS, issued a tile ahead. A team owns TEAM vertices of the tile and keeps
//               them side by side: per group, lane j issues the TEAM loads of piece j of their rows together, then folds each
//               into the two best (score, class) pairs of its vertex; the team's lanes then merge their pairs by a butterfly
//               (log2 TEAM steps of cross-lane reads). Pairs
//               compare by (score descending, class ascending) and every class is seen by exactly one lane, so the order is
//               total and the result does not depend on the order of merging. The labels of a tile are staged in LDS; then
//               thread t owns id tile * 256 + t: it reads prev[id], writes label / best / margin, and the tile's flips are
//               compacted in id order (ballot, popcount, mbcnt) into the workspace with the tile's count. A workgroup adds its
//               labels into an LDS histogram (integer adds: order-free) and flushes it once into the head's 64-bit counts.
//   k_as_scan   ONE workgroup: the exclusive scan of the tile counts in rounds of 256 tiles; n_flips and go = (n_flips <= cap),
//               decided here.
//   k_as_fill   returns at once unless go; copies every tile's compacted flips to base[tile] + rank.
//   k_as_at<TEAM>  the same row read and merge at m caller-given ids, one team per id.
// Every store is an ordinary vector store. -ffp-contract=off: a score is ONE multiplication, the margin ONE subtraction.
#pragma once

#include "dppr_common.hpp"
#include "dppr_assign_plan.hpp"

namespace dppr {

constexpr int AS_WAVES = AS_TILE / WAVE;
constexpr int AS_NONE = 0x7fffffff; // the class of an empty pair: loses every tie
static_assert(AS_TILE % WAVE == 0 && AS_TILE == 256, "a tile is a workgroup of four whole waves");

// the two best (score, class) pairs among the scores > +0.0 seen so far; an empty pair is (+0.0, AS_NONE)
struct AsTop2 {
    double s1, s2;
    int c1, c2;
};

__device__ __forceinline__ bool as_better(double a, int ca, double b, int cb) { return a > b || (a == b && ca < cb); }

// a class no pair of `t` holds yet
__device__ __forceinline__ void as_push(AsTop2 &t, double s, int c) {
    if (!(s > 0.0)) return; // (a negative score, +-0.0: neither a label nor a runner-up)
    if (as_better(s, c, t.s1, t.c1)) {
        t.s2 = t.s1;
        t.c2 = t.c1;
        t.s1 = s;
        t.c1 = c;
    } else if (as_better(s, c, t.s2, t.c2)) {
        t.s2 = s;
        t.c2 = c;
    }
}

// two sets of pairs over disjoint classes (scalars by value: the selects stay in registers)
__device__ __forceinline__ AsTop2 as_merge(double as1, int ac1, double as2, int ac2, double bs1, int bc1, double bs2, int bc2) {
    const bool a_first = as_better(as1, ac1, bs1, bc1);
    // the winner's second against the loser's first
    const double ws2 = a_first ? as2 : bs2, ls1 = a_first ? bs1 : as1;
    const int wc2 = a_first ? ac2 : bc2, lc1 = a_first ? bc1 : ac1;
    const bool keep = as_better(ws2, wc2, ls1, lc1);
    AsTop2 o;
    o.s1 = a_first ? as1 : bs1;
    o.c1 = a_first ? ac1 : bc1;
    o.s2 = keep ? ws2 : ls1;
    o.c2 = keep ? wc2 : lc1;
    return o;
}

// the pairs of a team's lanes merged, in every lane of the team (log2 TEAM steps of cross-lane reads). Called by all lanes of a wave.
template <int TEAM> __device__ __forceinline__ AsTop2 as_butterfly(AsTop2 t) {
#pragma unroll
    for (int s = 1; s < TEAM; s <<= 1) {
        const double os1 = __shfl_xor(t.s1, s), os2 = __shfl_xor(t.s2, s);
        const int oc1 = __shfl_xor(t.c1, s), oc2 = __shfl_xor(t.c2, s);
        t = as_merge(t.s1, t.c1, t.s2, t.c2, os1, oc1, os2, oc2);
    }
    return t;
}

// The pairs of the vertex in `row` (-1: none, every score is 0.0), in every lane of its team. Called by all lanes of a wave.
template <int TEAM> __device__ __forceinline__ AsTop2 as_vertex(const AsDesc &d, const double *__restrict__ scale, int row, int j) {
    AsTop2 t{0.0, 0.0, AS_NONE, AS_NONE};
    if (row >= 0) {
        for (int g = 0; g < d.n_groups; ++g) {
            const AsGroup gr = d.g[g];
            const double *pr = gr.p + (size_t)row * gr.gw; // (a group's rows are an even number of doubles wide: 16-byte loads)
            for (int h = j; 2 * h < gr.n; h += TEAM) {
                const double2 v = *reinterpret_cast<const double2 *>(pr + 2 * h);
                const int c = gr.base + 2 * h;
                as_push(t, scale ? scale[c] * v.x : v.x, c);
                if (2 * h + 1 < gr.n) as_push(t, scale ? scale[c + 1] * v.y : v.y, c + 1);
            }
        }
    }
    return as_butterfly<TEAM>(t);
}

// what the definition of include/dppr.h makes of the pairs
struct AsResult {
    int label, second_label;
    double best, margin;
};
__device__ __forceinline__ AsResult as_result(const AsTop2 &t, double min_score) {
    AsResult r;
    if (t.s1 > min_score) {
        r.label = t.c1;
        r.second_label = t.c2 == AS_NONE ? -1 : t.c2;
        r.best = t.s1;
        r.margin = t.s1 - t.s2;
    } else { // (no class is the label, so none is left out of the runner-up: the largest positive score, if there is one)
        r.label = -1;
        r.second_label = t.c1 == AS_NONE ? -1 : t.c1;
        r.best = 0.0;
        r.margin = 0.0;
    }
    return r;
}

// out_label [V] always; out_best / out_margin [V] or NULL; prev [V] or NULL (may BE out_label: thread t reads prev[id] before
// it writes out_label[id]). cnt [tiles] and ws (three planes of `plane` ints) are written only with prev. counts: [C + 1],
// zeroed by the caller.
template <int TEAM>
__global__ __launch_bounds__(AS_TILE) void k_as_label(const AsDesc d, const double *__restrict__ scale, double min_score,
                                                      const int *__restrict__ ext2int, int V, const int *prev, int *out_label,
                                                      double *__restrict__ out_best, double *__restrict__ out_margin,
                                                      int *__restrict__ cnt, int *__restrict__ ws, size_t plane,
                                                      unsigned long long *__restrict__ counts) {
    __shared__ int s_row[AS_TILE], s_label[AS_TILE];
    __shared__ double s_best[AS_TILE], s_margin[AS_TILE];
    __shared__ int s_hist[AS_CLASSES_MAX + 1];
    __shared__ int s_w[AS_WAVES];
    constexpr int PER = AS_TILE / TEAM; // vertices a workgroup reads per step
    const int j = (int)threadIdx.x % TEAM, slot = (int)threadIdx.x / TEAM;
    const int tiles = (V + AS_TILE - 1) / AS_TILE;
    for (int c = threadIdx.x; c <= AS_CLASSES_MAX; c += AS_TILE) s_hist[c] = 0;
    __syncthreads();
    // one coalesced read of a tile's rows, issued a tile ahead: it is in flight while the tile before it is reduced
    auto row_of = [&](int tile) {
        if (tile >= tiles) return -1;
        const int ext = tile * AS_TILE + (int)threadIdx.x;
        return ext < V ? ext2int[ext] : -1;
    };
    int ahead = row_of(blockIdx.x);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        s_row[threadIdx.x] = ahead;
        ahead = row_of(tile + (int)gridDim.x);
        const int own = tile * AS_TILE + (int)threadIdx.x;
        const int old_label = prev && own < V ? prev[own] : 0; // (read by the thread that writes label[own] below; early: beside the row loads)
        __syncthreads();
        // the TEAM vertices of this thread's team, one per step, side by side: per group their TEAM row loads are in flight together
        AsTop2 t[TEAM];
        int row[TEAM];
#pragma unroll
        for (int step = 0; step < TEAM; ++step) {
            t[step] = AsTop2{0.0, 0.0, AS_NONE, AS_NONE};
            row[step] = s_row[step * PER + slot];
        }
        for (int g = 0; g < d.n_groups; ++g) {
            const AsGroup gr = d.g[g];
            // (as_team: 2 TEAM >= the widest row, so piece j is the only piece of this lane)
            const bool mine = 2 * j < gr.n, two = 2 * j + 1 < gr.n;
            const int c = gr.base + 2 * j;
            double sc0 = 1.0, sc1 = 1.0;
            if (scale && mine) {
                sc0 = scale[c];
                if (two) sc1 = scale[c + 1];
            }
            double2 v[TEAM];
#pragma unroll
            for (int step = 0; step < TEAM; ++step)
                v[step] = mine && row[step] >= 0 ? *reinterpret_cast<const double2 *>(gr.p + (size_t)row[step] * gr.gw + 2 * j) : make_double2(0.0, 0.0);
#pragma unroll
            for (int step = 0; step < TEAM; ++step) {
                as_push(t[step], scale ? sc0 * v[step].x : v[step].x, c);
                if (two) as_push(t[step], scale ? sc1 * v[step].y : v[step].y, c + 1);
            }
        }
#pragma unroll
        for (int step = 0; step < TEAM; ++step) {
            const AsTop2 m = as_butterfly<TEAM>(t[step]);
            if (j == 0) {
                const AsResult r = as_result(m, min_score);
                const int il = step * PER + slot;
                s_label[il] = r.label;
                s_best[il] = r.best;
                s_margin[il] = r.margin;
            }
        }
        __syncthreads();
        const int ext = own;
        const bool in = ext < V;
        const int lab = s_label[threadIdx.x];
        const int old = prev ? old_label : lab;
        if (in) {
            out_label[ext] = lab;
            if (out_best) out_best[ext] = s_best[threadIdx.x];
            if (out_margin) out_margin[ext] = s_margin[threadIdx.x];
            if (lab >= 0) atomicAdd(&s_hist[lab], 1);
        }
        { // the unassigned of a wave in one add (most ids of a sparse window: 64 lanes on one LDS word would take turns)
            const uint64_t un = __ballot(in && lab < 0);
            if (lane_id() == 0 && un) atomicAdd(&s_hist[d.C], __popcll(un));
        }
        if (prev) { // (the same in every thread)
            const bool flip = in && old != lab;
            const uint64_t b = __ballot(flip);
            if (lane_id() == 0) s_w[wave_id()] = __popcll(b);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int k = 0; k < AS_WAVES; ++k) {
                before += k < wave_id() ? s_w[k] : 0;
                total += s_w[k];
            }
            if (flip) {
                const size_t at = (size_t)tile * AS_TILE + (size_t)(before + mbcnt(b));
                ws[at] = ext;
                ws[plane + at] = old;
                ws[2 * plane + at] = lab;
            }
            if (threadIdx.x == 0) cnt[tile] = total;
        }
        __syncthreads(); // (the staged labels and the wave counts are read before the next tile overwrites them)
    }
    for (int c = threadIdx.x; c <= d.C; c += AS_TILE)
        if (s_hist[c]) atomicAdd(&counts[c], (unsigned long long)s_hist[c]);
}

// One workgroup of AS_TILE threads. base [tiles]; head->n_flips, head->go.
__global__ __launch_bounds__(AS_TILE) void k_as_scan(const int *__restrict__ cnt, int tiles, long long cap, int *__restrict__ base,
                                                     AsHead *__restrict__ head) {
    __shared__ int s_w[AS_WAVES];
    long long carry = 0; // (the same in every thread)
    for (int t0 = 0; t0 < tiles; t0 += AS_TILE) {
        const int t = t0 + (int)threadIdx.x;
        const int c = t < tiles ? cnt[t] : 0;
        const int inc = wave_inclusive_scan(c);
        if (lane_id() == WAVE - 1) s_w[wave_id()] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < AS_WAVES; ++k) {
            before += k < wave_id() ? s_w[k] : 0;
            total += s_w[k];
        }
        if (t < tiles) base[t] = (int)carry + before + (inc - c); // (at most one flip per vertex: inside an int)
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        head->n_flips = carry;
        head->go = carry <= cap ? 1 : 0;
        head->pad = 0;
    }
}

// flip_id / flip_old / flip_new: head->n_flips entries each, written only if head->go
__global__ __launch_bounds__(AS_TILE) void k_as_fill(const int *__restrict__ cnt, const int *__restrict__ base,
                                                     const int *__restrict__ ws, size_t plane, int tiles,
                                                     const AsHead *__restrict__ head, int *__restrict__ flip_id,
                                                     int *__restrict__ flip_old, int *__restrict__ flip_new) {
    if (!head->go) return;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if ((int)threadIdx.x < cnt[tile]) {
            const size_t from = (size_t)tile * AS_TILE + threadIdx.x, to = (size_t)base[tile] + threadIdx.x;
            flip_id[to] = ws[from];
            flip_old[to] = ws[plane + from];
            flip_new[to] = ws[2 * plane + from];
        }
    }
}

// out_val: [m][2] = (best, margin); out_lab: 16 bytes per id, the first 8 = (label, second_label)
template <int TEAM>
__global__ __launch_bounds__(AS_TILE) void k_as_at(const AsDesc d, const double *__restrict__ scale, double min_score,
                                                   const int *__restrict__ ext2int, const int *__restrict__ ids, int m,
                                                   double *__restrict__ out_val, int *__restrict__ out_lab) {
    constexpr int PER = AS_TILE / TEAM;
    const int j = (int)threadIdx.x % TEAM, slot = (int)threadIdx.x / TEAM;
    for (int i0 = blockIdx.x * PER; i0 < m; i0 += gridDim.x * PER) { // (the same trip count in every lane of a wave)
        const int i = i0 + slot;
        const int row = i < m ? ext2int[ids[i]] : -1;
        const AsTop2 t = as_vertex<TEAM>(d, scale, row, j);
        if (i < m && j == 0) {
            const AsResult r = as_result(t, min_score);
            out_val[2 * (size_t)i] = r.best;
            out_val[2 * (size_t)i + 1] = r.margin;
            out_lab[4 * (size_t)i] = r.label;
            out_lab[4 * (size_t)i + 1] = r.second_label;
        }
    }
}

} // namespace dppr
