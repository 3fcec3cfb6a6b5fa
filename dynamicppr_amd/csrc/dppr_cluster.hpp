// dppr_cluster.hpp -- the conductance sweep over a top-k order (dppr_cluster, dppr_group_cluster). Never called from the update path.
//
// The selection of dppr_topk.hpp leaves, per lane i, the order v_0 .. v_{L-1} (external ids, [n][k]) and L on the device. With
// rho_i(w) the position of w in lane i's order (absent: above every position), the cut of prefix S_j changes by what v_j brings:
// v_j's edges to vertices NOT yet inside start to cross, the edges of vertices already inside TO v_j stop crossing. Per position
//     d_out[j] = #{out-neighbours w of v_j : rho(w) > j} - #{in-neighbours  w of v_j : rho(w) < j}
//     d_in[j]  = #{in-neighbours  w of v_j : rho(w) > j} - #{out-neighbours w of v_j : rho(w) < j}
//     deg[j]   = length of v_j's out-row
// (entries of equal rank are self loops and in neither count; rows count duplicates as often as they are stored), and the
// inclusive prefix sums of the three are cut_out, cut_in and vol of include/dppr.h.
//
//   k_cl_rank   scatters j into the rank table: one uint16 per (occupied row, lane), rows of cl_stride(n) entries, cleared to
//               CL_ABSENT (0xffff) by a memset per call
//   k_cl_rows   one wave per (lane, position): the bounds of both rows through readfirstlane, the rows read coalesced 64
//               entries at a time, one gather of a rank per entry, the two counts kept wave-uniform (popcount of a ballot). A row
//               of more than CL_SPLIT entries -- a prefix of a PPR order holds the hubs -- is not walked here: the wave queues
//               its chunks of CL_SPLIT entries (one global add reserves the range)
//   k_cl_big    one wave per queued chunk, from a fixed grid; its two counts join d_out / d_in by one integer vector atomic each.
//               Integer sums: the result does not depend on the order in which the chunks arrive
//   k_cl_scan   one workgroup per lane: inclusive scan of the three arrays in LDS (64-bit sums), den, phi = one division, the
//               first minimum over the eligible positions; writes the lane's record and its rows of the three arrays
// Nothing is read back between the kernels; every result is written with ordinary vector stores.
#pragma once

#include "dppr_cluster_plan.hpp"
#include "dppr_common.hpp"
#include "dppr_topk.hpp"

namespace dppr {

struct ClGraph {              // the epoch's two CSRs by internal id, and where the occupied rows lie
    const int *out_row_ptr, *out_col;
    const int *in_row_ptr;
    const Adj *in_adj;
    int n_int, lo_parked, rows; // live zone [0, n_int), parked zone [lo_parked, lo_parked + rows - n_int)
};

struct ClCtl {                // zeroed per call
    unsigned n_items;         // chunk items queued by k_cl_rows
    unsigned pad[3];
};

// index of internal id w among the occupied rows (-1: w lies in neither zone)
__device__ __forceinline__ int cl_row_index(const ClGraph &g, int w) {
    if ((unsigned)w < (unsigned)g.n_int) return w;
    const int q = g.n_int + (w - g.lo_parked);
    return (w >= g.lo_parked && q < g.rows) ? q : -1;
}
__device__ __forceinline__ int cl_rank_of(const ClGraph &g, const unsigned short *__restrict__ rank, int stride, int lane, int w) {
    const int q = cl_row_index(g, w);
    return q >= 0 ? (int)rank[(size_t)q * stride + lane] : CL_ABSENT;
}

// grid: ceil(n * k / 256). ids [n][k] external (-1 past the count)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_rank(ClGraph g, const int *__restrict__ ext2int, const int *__restrict__ cnt,
                                                      const int *__restrict__ ids, int n, int k, int stride,
                                                      unsigned short *__restrict__ rank) {
    const int t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n * k) return;
    const int lane = t / k, j = t - lane * k;
    if (j >= min(cnt[lane], k)) return;
    const int q = cl_row_index(g, ext2int[ids[t]]);
    if (q >= 0) rank[(size_t)q * stride + lane] = (unsigned short)j;
}

// entries [lo, hi) of a row (DIR 0: out_col, 1: in_adj) against position j: how many neighbours rank above it, how many below
template <int DIR>
__device__ __forceinline__ void cl_walk(const ClGraph &g, const unsigned short *__restrict__ rank, int stride, int lane, int j, int lo,
                                        int hi, int *gt, int *lt) {
    int a = 0, b = 0;
    for (int e0 = lo; e0 < hi; e0 += WAVE) {
        const int e = e0 + lane_id();
        int rho = j; // (a lane past the end: in neither count)
        if (e < hi) rho = cl_rank_of(g, rank, stride, lane, DIR == 0 ? ld_stream(g.out_col + e) : g.in_adj[e].v);
        a += __popcll(__ballot(rho > j));
        b += __popcll(__ballot(rho < j));
    }
    *gt = a;
    *lt = b;
}

// grid: ceil(n * k / 4), one wave per (lane, position). d: d_out [n][k] | d_in [n][k] | deg [n][k]
__global__ __launch_bounds__(CL_BLOCK) void k_cl_rows(ClGraph g, const int *__restrict__ ext2int, const int *__restrict__ cnt,
                                                      const int *__restrict__ ids, int n, int k, int stride,
                                                      const unsigned short *__restrict__ rank, int *__restrict__ d, ClCtl *__restrict__ ctl,
                                                      unsigned long long *__restrict__ list, unsigned list_cap) {
    const int pos = blockIdx.x * CL_WAVES + wave_id();
    if (pos >= n * k) return;
    const int lane = pos / k, j = pos - lane * k;
    const size_t nk = (size_t)n * (size_t)k;
    int d_out = 0, d_in = 0, deg = 0;
    if (j < min(cnt[lane], k)) {
        const int u = __builtin_amdgcn_readfirstlane(ext2int[ids[pos]]);
        if (u >= 0) { // (a vertex of the order has a row of the state: always)
            const int o0 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u]), o1 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u + 1]);
            const int i0 = __builtin_amdgcn_readfirstlane(g.in_row_ptr[u]), i1 = __builtin_amdgcn_readfirstlane(g.in_row_ptr[u + 1]);
            deg = o1 - o0;
            int gt = 0, lt = 0;
            unsigned queued = 0; // chunks this wave hands to k_cl_big: those of its out-row, then those of its in-row
            const unsigned c_out = o1 - o0 > CL_SPLIT ? (unsigned)cl_chunks(o1 - o0) : 0u;
            const unsigned c_in = i1 - i0 > CL_SPLIT ? (unsigned)cl_chunks(i1 - i0) : 0u;
            if (!c_out) {
                cl_walk<0>(g, rank, stride, lane, j, o0, o1, &gt, &lt);
                d_out += gt;
                d_in -= lt;
            }
            if (!c_in) {
                cl_walk<1>(g, rank, stride, lane, j, i0, i1, &gt, &lt);
                d_in += gt;
                d_out -= lt;
            }
            queued = c_out + c_in;
            if (queued) {
                unsigned base = 0;
                if (lane_id() == 0) base = atomicAdd(&ctl->n_items, queued);
                base = __builtin_amdgcn_readfirstlane(base);
                for (unsigned c = lane_id(); c < queued; c += WAVE)
                    if (base + c < list_cap) // (cl_list_cap bounds what a call can queue)
                        list[base + c] = c < c_out ? cl_item((unsigned)pos, 0u, c) : cl_item((unsigned)pos, 1u, c - c_out);
            }
        }
    }
    if (lane_id() == 0) {
        d[pos] = d_out;
        d[nk + pos] = d_in;
        d[2 * nk + pos] = deg;
    }
}

// fixed grid, one wave per queued chunk
__global__ __launch_bounds__(CL_BLOCK) void k_cl_big(ClGraph g, const int *__restrict__ ext2int, const int *__restrict__ ids, int n, int k,
                                                     int stride, const unsigned short *__restrict__ rank, int *__restrict__ d,
                                                     const ClCtl *__restrict__ ctl, const unsigned long long *__restrict__ list,
                                                     unsigned list_cap) {
    const unsigned n_items = min(ctl->n_items, list_cap);
    const size_t nk = (size_t)n * (size_t)k;
    for (unsigned t = blockIdx.x * CL_WAVES + wave_id(); t < n_items; t += gridDim.x * CL_WAVES) {
        const unsigned long long it = list[t];
        const int pos = (int)cl_item_pos(it), dir = (int)cl_item_dir(it);
        const int lane = pos / k, j = pos - lane * k;
        const int u = __builtin_amdgcn_readfirstlane(ext2int[ids[pos]]);
        const int *rp = dir ? g.in_row_ptr : g.out_row_ptr;
        const int r0 = __builtin_amdgcn_readfirstlane(rp[u]), r1 = __builtin_amdgcn_readfirstlane(rp[u + 1]);
        const long long lo = (long long)r0 + (long long)cl_item_chunk(it) * CL_SPLIT;
        const int hi = (int)min((long long)r1, lo + CL_SPLIT);
        int gt = 0, lt = 0;
        if (lo < hi) {
            if (dir) cl_walk<1>(g, rank, stride, lane, j, (int)lo, hi, &gt, &lt);
            else cl_walk<0>(g, rank, stride, lane, j, (int)lo, hi, &gt, &lt);
        }
        if (lane_id() == 0) {
            // out-row: (+gt, -lt) into (d_out, d_in); in-row: (-lt, +gt)
            const int add_out = dir ? -lt : gt, add_in = dir ? gt : -lt;
            if (add_out) atomicAdd(&d[pos], add_out);
            if (add_in) atomicAdd(&d[nk + pos], add_in);
        }
    }
}

// inclusive scan of one 64-bit value per thread over the workgroup; s_w: one word per wave
__device__ __forceinline__ long long cl_block_scan(long long x, long long *s_w) {
    // inside the wave: Hillis-Steele over the lanes
    for (int dlt = 1; dlt < WAVE; dlt <<= 1) {
        const long long y = __shfl_up(x, dlt, WAVE);
        if (lane_id() >= dlt) x += y;
    }
    __syncthreads(); // (s_w of the previous scan has been read)
    if (lane_id() == WAVE - 1) s_w[wave_id()] = x;
    __syncthreads();
    long long before = 0;
    for (int w = 0; w < wave_id(); ++w) before += s_w[w];
    return x + before;
}

// grid: n, one workgroup per lane. best [16]; out_cut_out / out_cut_in / out_vol [n][k]
__global__ __launch_bounds__(CL_SCAN_BLOCK) void k_cl_scan(const int *__restrict__ cnt, const int *__restrict__ d, int n, int k, long long Ed,
                                                           int min_size, dppr_cluster_t *__restrict__ best, long long *__restrict__ out_cut_out,
                                                           long long *__restrict__ out_cut_in, long long *__restrict__ out_vol) {
    __shared__ long long s_w[CL_SCAN_BLOCK / WAVE];
    __shared__ double s_phi[CL_SCAN_BLOCK / WAVE];
    __shared__ int s_j[CL_SCAN_BLOCK / WAVE];
    const int lane = blockIdx.x, tid = threadIdx.x;
    const int L = min(cnt[lane], k);
    const size_t nk = (size_t)n * (size_t)k, o = (size_t)lane * (size_t)k;
    const int j0 = tid * CL_PER_THREAD;
    long long v[3][CL_PER_THREAD];
    long long tot[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int t = 0; t < CL_PER_THREAD; ++t) {
            const int j = j0 + t;
            tot[a] += j < L ? (long long)d[a * nk + o + j] : 0ll;
            v[a][t] = tot[a]; // (inclusive inside the thread)
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long long before = cl_block_scan(tot[a], s_w) - tot[a];
#pragma unroll
        for (int t = 0; t < CL_PER_THREAD; ++t) v[a][t] += before;
    }
    double phi = __builtin_huge_val();
    int bj = -1;
    long long bcut = 0, bvol = 0;
#pragma unroll
    for (int t = 0; t < CL_PER_THREAD; ++t) {
        const int j = j0 + t;
        if (j < k) {
            out_cut_out[o + j] = j < L ? v[0][t] : 0ll;
            out_cut_in[o + j] = j < L ? v[1][t] : 0ll;
            out_vol[o + j] = j < L ? v[2][t] : 0ll;
        }
        if (j < L && j + 1 >= min_size) {
            const long long vol = v[2][t], den = min(vol, Ed - vol);
            if (den > 0) {
                const double f = __ddiv_rn((double)v[0][t], (double)den);
                if (bj < 0 || f < phi) { // (ascending j: the first of equal values stays)
                    phi = f;
                    bj = j;
                    bcut = v[0][t];
                    bvol = vol;
                }
            }
        }
    }
    // the workgroup's first minimum: (phi, j) ascending; a thread without an eligible position holds (+inf, INT_MAX)
    int key_j = bj < 0 ? 0x7fffffff : bj;
    double wphi = phi;
    int wj = key_j;
    for (int dlt = 1; dlt < WAVE; dlt <<= 1) {
        const double p2 = __shfl_xor(wphi, dlt, WAVE);
        const int j2 = __shfl_xor(wj, dlt, WAVE);
        if (p2 < wphi || (p2 == wphi && j2 < wj)) {
            wphi = p2;
            wj = j2;
        }
    }
    if (lane_id() == 0) {
        s_phi[wave_id()] = wphi;
        s_j[wave_id()] = wj;
    }
    __syncthreads();
    for (int w = 0; w < CL_SCAN_BLOCK / WAVE; ++w) // (every thread: the same loop, the same winner)
        if (s_phi[w] < wphi || (s_phi[w] == wphi && s_j[w] < wj)) {
            wphi = s_phi[w];
            wj = s_j[w];
        }
    const bool any = wj != 0x7fffffff;
    if (any ? (bj == wj) : tid == 0) { // the thread that owns the winner writes the record (none eligible: thread 0)
        dppr_cluster_t b;
        b.count = L;
        b.best_size = any ? bj + 1 : 0;
        b.best_cut = any ? bcut : 0;
        b.best_vol = any ? bvol : 0;
        b.best_phi = any ? phi : __builtin_huge_val();
        best[lane] = b;
    }
}

} // namespace dppr
