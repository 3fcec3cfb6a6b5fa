// dppr_dot.hpp -- the state folded over the VERTEX axis: out[f][i] = fold_j (h_f[slot j] * x_i[vertex of slot j]), x = p or r of
// lane i by external id (dppr_dot_dense_dev / dppr_dot_sparse and their group forms). Never called from the update path.
//
// THE FOLD is that of include/dppr.h: every product __dmul_rn, every sum __dadd_rn, blocks of 2^16 slots summed by the balanced
// tree that adds neighbours, the blocks added in ascending order. dppr_dot_plan.hpp cuts the tree into subtile (256 slots), tile
// (8 subtiles) and block (32 tiles); where the pieces meet is fixed by the slot number alone, so the result does not depend on
// the grid, on F, on n or on how the features are chunked. Padding is +0.0 and is ADDED (-0.0 + +0.0 = +0.0): a subtile or a tile
// of pure padding is the value +0.0 without work, nothing else is skipped.
//
// DENSE  k_dot_dense<T, VERTEX_MAJOR>: a workgroup takes tiles of 2048 external ids, blockIdx.y a chunk of <= 16 features. Per
//   subtile: row = ext2int[ext]; the gw-wide rows gathered once (16-byte loads where gw is even, 8-byte loads on a slot) into LDS
//   rows padded by one double (the bank argument of dppr_wquery.hpp: threads of a wave read lanes of one row, or rows an odd number
//   of doubles apart); the h tile read coalesced -- feature-major: consecutive threads, consecutive ids of one feature;
//   vertex-major: consecutive threads, consecutive addresses, transposed on the way into LDS -- f32 widened on load (exact).
//   The tree: outputs = features x lanes <= 256; the subtile's slots are split over G = 256 / outputs (a power of two) thread groups
//   along subtree boundaries, thread (g, f, i) folds its 256 / G slots in registers (dot_leaf: a binary counter of partial sums
//   with static indices, the left operand always the earlier slots), the G sums meet by neighbours in LDS. Thread (0, f, i)
//   carries the subtile sums through the same counter and stores ONE partial per (tile, f, i).
// SPARSE k_dot_sparse: the same fold over the tile table of the call (dppr_dot_plan.hpp): one thread per entry reads its id and
//   weight and gathers the row at ext2int[id]. An id outside [0, V) reads nothing and raises head->bad.
// COMBINE k_dot_combine: one wave per output: lane b folds the 32 partials of block b (static tree in registers), the blocks are
//   added in ascending order (acc = B_0; acc = acc + B_b), lane 0 writes -- unless head->bad (as k_ex_fill is gated on go).
// Every store is an ordinary vector store; there is no atomic: every position and every order is fixed by construction.
#pragma once

#include "dppr_common.hpp"
#include "dppr_dot_plan.hpp"

namespace dppr {

constexpr int DOT_HS = DOT_TILE + 1; // doubles between two features of the h tile in LDS

template <class T> __device__ __forceinline__ double dot_widen(T v) { return (double)v; } // (f32 -> f64 is exact)

// the subtree over slots [s0, s0 + L) of the staged subtile, L a power of two: h[s] * x[s * ls]. Eight slots a step where L allows:
// sixteen independent LDS reads in flight and a static three-level tree, then the counter over the steps (a thread of the widest
// pass folds 256 slots on its own: what it waits for is latency, not bandwidth)
__device__ __forceinline__ double dot_leaf(const double *h, const double *x, int ls, int s0, int L) {
    if (L == 1) return __dmul_rn(h[s0], x[s0 * ls]);
    double v = 0.0;
    if (L < 8) { // 2 or 4 slots: pairs, and one level above them
        double first = 0.0;
        for (int j = 0; 2 * j < L; ++j) {
            const int s = s0 + 2 * j;
            v = __dadd_rn(__dmul_rn(h[s], x[s * ls]), __dmul_rn(h[s + 1], x[(s + 1) * ls]));
            if (j == 0)
                first = v;
            else
                v = __dadd_rn(first, v);
        }
        return v;
    }
    double lvl[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; 8 * j < L; ++j) {
        const int s = s0 + 8 * j;
        double t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = __dmul_rn(h[s + k], x[(s + k) * ls]);
        v = __dadd_rn(__dadd_rn(__dadd_rn(t[0], t[1]), __dadd_rn(t[2], t[3])), __dadd_rn(__dadd_rn(t[4], t[5]), __dadd_rn(t[6], t[7])));
        bool carry = true; // (j is the same in every thread: the branches below are scalar)
#pragma unroll
        for (int k = 0; k < 5; ++k) { // level k + 4: the sum of eight meets the sum of the 2^(k+3) slots before it
            const bool bit = (j >> k) & 1;
            if (carry && bit) {
                v = __dadd_rn(lvl[k], v);
            } else if (carry) {
                lvl[k] = v;
                carry = false;
            }
        }
    }
    return v; // (the last step carried through every level below L)
}

// The staged subtile folded for every output: thread tid = g * outs + o takes subtree g of output o = fl * n + i; the sum of the whole
// subtile comes back in the threads tid < outs. Called by the whole workgroup.
__device__ __forceinline__ double dot_subtile(const double *s_h, const double *s_x, double *s_part, int ls, int n, int outs, int G) {
    const int tid = (int)threadIdx.x, L = DOT_TILE / G;
    const bool on = tid < G * outs;
    const int g = tid / outs, o = tid % outs;
    if (on) s_part[tid] = dot_leaf(s_h + (o / n) * DOT_HS, s_x + (o % n), ls, g * L, L);
    for (int step = 1; step < G; step <<= 1) {
        __syncthreads();
        if (on && (g & (2 * step - 1)) == 0) s_part[tid] = __dadd_rn(s_part[tid], s_part[tid + step * outs]);
    }
    return on ? s_part[tid] : 0.0;
}

// the subtile sums of a tile, in slot order, through the counter: the value after the last one is the tile's
struct DotCarry {
    double l0 = 0.0, l1 = 0.0, l2 = 0.0;
    static_assert(DOT_SUB == 8, "three levels above a subtile");
    __device__ __forceinline__ double push(int sub, double v) {
        if (!(sub & 1)) {
            l0 = v;
            return v;
        }
        v = __dadd_rn(l0, v);
        if (!(sub & 2)) {
            l1 = v;
            return v;
        }
        v = __dadd_rn(l1, v);
        if (!(sub & 4)) {
            l2 = v;
            return v;
        }
        return __dadd_rn(l2, v);
    }
};

__device__ __forceinline__ int dot_groups_dev(int outs) {
    int g = 1;
    while (2 * g * outs <= DOT_TILE) g *= 2;
    return g;
}

// rows of s_row[0 .. DOT_TILE) into s_x (a row < 0: zeros)
__device__ __forceinline__ void dot_gather_rows(const double *__restrict__ x, int gw, const int *s_row, double *s_x) {
    const int ls = gw + 1;
    if (gw & 1) { // a single-source slot: rows of one double
        for (int j = threadIdx.x; j < DOT_TILE * gw; j += DOT_TILE) {
            const int il = j / gw, l = j % gw, row = s_row[il];
            s_x[il * ls + l] = row >= 0 ? x[(size_t)row * gw + l] : 0.0;
        }
    } else {
        const int half = gw / 2;
        for (int j = threadIdx.x; j < DOT_TILE * half; j += DOT_TILE) {
            const int il = j / half, hh = j % half, row = s_row[il];
            double2 v = make_double2(0.0, 0.0);
            if (row >= 0) v = *reinterpret_cast<const double2 *>(x + (size_t)row * gw + 2 * hh);
            s_x[il * ls + 2 * hh] = v.x;
            s_x[il * ls + 2 * hh + 1] = v.y;
        }
    }
}

// x: p or r of the state (rows of gw doubles, n lanes in use). h: [F][V] or, VMAJOR, [V][F]. Features [f0, f1) of this launch,
// chunk blockIdx.y of them; fcm: features the LDS was sized for. part[((f - f0) * n + i) * stride + tile].
template <class T, bool VMAJOR>
__global__ __launch_bounds__(DOT_TILE) void k_dot_dense(const double *__restrict__ x, int gw, int n, const int *__restrict__ ext2int,
                                                        int V, const T *__restrict__ h, int F, int f0, int f1, int fcm,
                                                        double *__restrict__ part, long long stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dot_lds[];
    const int ls = gw + 1, tid = (int)threadIdx.x;
    double *s_x = reinterpret_cast<double *>(dot_lds);
    double *s_h = s_x + DOT_TILE * ls;
    double *s_part = s_h + fcm * DOT_HS;
    int *s_row = reinterpret_cast<int *>(s_part + DOT_TILE);
    const int fb = f0 + (int)blockIdx.y * DOT_FCHUNK, fc = min(DOT_FCHUNK, f1 - fb);
    const int outs = fc * n, G = dot_groups_dev(outs);
    const long long tiles = ((long long)V + DOT_WG_SLOTS - 1) / DOT_WG_SLOTS;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        DotCarry carry;
        double sum = 0.0;
        for (int sub = 0; sub < DOT_SUB; ++sub) {
            const long long e0 = tile * DOT_WG_SLOTS + (long long)sub * DOT_TILE;
            const int cnt = (int)min((long long)DOT_TILE, (long long)V - e0);
            double v = 0.0; // (a subtile of padding)
            if (cnt > 0) {
                __syncthreads(); // (the fold of the previous subtile is over)
                s_row[tid] = tid < cnt ? ext2int[e0 + tid] : -1;
                if constexpr (!VMAJOR) {
                    for (int fl = 0; fl < fc; ++fl)
                        s_h[fl * DOT_HS + tid] = tid < cnt ? dot_widen(h[(size_t)(fb + fl) * (size_t)V + (size_t)(e0 + tid)]) : 0.0;
                } else {
                    for (int j = tid; j < DOT_TILE * fc; j += DOT_TILE) {
                        const int il = j / fc, fl = j % fc;
                        s_h[fl * DOT_HS + il] = il < cnt ? dot_widen(h[(size_t)(e0 + il) * (size_t)F + (size_t)(fb + fl)]) : 0.0;
                    }
                }
                __syncthreads();
                dot_gather_rows(x, gw, s_row, s_x);
                __syncthreads();
                v = dot_subtile(s_h, s_x, s_part, ls, n, outs, G);
            }
            sum = carry.push(sub, v);
        }
        if (tid < outs) part[((size_t)blockIdx.y * DOT_FCHUNK * n + tid) * (size_t)stride + (size_t)tile] = sum;
    }
}

// ids / w: the entries of the call; tiles: its table. part[i * stride + col].
__global__ __launch_bounds__(DOT_TILE) void k_dot_sparse(const double *__restrict__ x, int gw, int n, const int *__restrict__ ext2int,
                                                         int V, const int *__restrict__ ids, const double *__restrict__ w,
                                                         const DotTile *__restrict__ tiles, long long n_tiles,
                                                         DotHead *__restrict__ head, double *__restrict__ part, long long stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dot_lds[];
    const int ls = gw + 1, tid = (int)threadIdx.x;
    double *s_x = reinterpret_cast<double *>(dot_lds);
    double *s_h = s_x + DOT_TILE * ls;
    double *s_part = s_h + DOT_HS;
    const int G = dot_groups_dev(n);
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const DotTile tl = tiles[t];
        DotCarry carry;
        double sum = 0.0;
        for (int sub = 0; sub < DOT_SUB; ++sub) {
            const int cnt = min(DOT_TILE, tl.cnt - sub * DOT_TILE);
            double v = 0.0; // (a subtile of padding)
            if (cnt > 0) {
                __syncthreads(); // (the fold of the previous subtile is over)
                int row = -1;
                double wv = 0.0;
                if (tid < cnt) {
                    const long long e = tl.e0 + (long long)sub * DOT_TILE + tid;
                    const int id = ids[e];
                    wv = w[e];
                    if ((unsigned)id < (unsigned)V)
                        row = ext2int[id];
                    else
                        head->bad = 1; // (every writer stores the same word; the combine launch reads it)
                }
                s_h[tid] = wv;
                double *dst = s_x + tid * ls;
                if (gw & 1) {
                    for (int l = 0; l < gw; ++l) dst[l] = row >= 0 ? x[(size_t)row * gw + l] : 0.0;
                } else {
                    for (int hh = 0; 2 * hh < gw; ++hh) {
                        double2 r2 = make_double2(0.0, 0.0);
                        if (row >= 0) r2 = *reinterpret_cast<const double2 *>(x + (size_t)row * gw + 2 * hh);
                        dst[2 * hh] = r2.x;
                        dst[2 * hh + 1] = r2.y;
                    }
                }
                __syncthreads();
                v = dot_subtile(s_h, s_x, s_part, ls, n, n, G);
            }
            sum = carry.push(sub, v);
        }
        if (tid < n) part[(size_t)tid * (size_t)stride + (size_t)tl.col] = sum;
    }
}

constexpr int DOT_CB_WAVES = 4; // outputs of a workgroup of the combine launch

// col == nullptr (dense): output q folds part[q * stride ..), stride / 32 blocks. Otherwise (sparse) q = f * n + i folds the blocks
// col[f] .. col[f + 1] of part[i * stride ..). out[q]; nothing is written if head->bad.
__global__ __launch_bounds__(DOT_CB_WAVES *WAVE) void k_dot_combine(const double *__restrict__ part, const long long *__restrict__ col,
                                                                     long long stride, int nout, int n,
                                                                     const DotHead *__restrict__ head, double *__restrict__ out) {
    const int q = (int)blockIdx.x * DOT_CB_WAVES + wave_id(), li = lane_id();
    if (q >= nout || head->bad) return; // (the same in every lane of the wave)
    long long base, nblk;
    if (col) {
        const int f = q / n, i = q % n;
        base = (long long)i * stride + col[f];
        nblk = (col[f + 1] - col[f]) / DOT_TPB;
    } else {
        base = (long long)q * stride;
        nblk = stride / DOT_TPB;
    }
    double acc = 0.0; // (a query without slots)
    for (long long b0 = 0; b0 < nblk; b0 += WAVE) {
        double B = 0.0;
        if (b0 + li < nblk) {
            const double2 *src = reinterpret_cast<const double2 *>(part + base + (b0 + li) * DOT_TPB);
            double y[DOT_TPB];
#pragma unroll
            for (int j = 0; j < DOT_TPB / 2; ++j) {
                const double2 v = src[j];
                y[2 * j] = v.x;
                y[2 * j + 1] = v.y;
            }
#pragma unroll
            for (int len = DOT_TPB; len > 1; len /= 2)
#pragma unroll
                for (int j = 0; j < len / 2; ++j) y[j] = __dadd_rn(y[2 * j], y[2 * j + 1]);
            B = y[0];
        }
        const int m = (int)min((long long)WAVE, nblk - b0);
        for (int k = 0; k < m; ++k) {
            const double Bk = __shfl(B, k);
            acc = (b0 == 0 && k == 0) ? Bk : __dadd_rn(acc, Bk);
        }
    }
    if (li == 0) out[q] = acc;
}

} // namespace dppr
