// dppr_subgraph.hpp -- the subgraph a top-k order induces (dppr_subgraph, dppr_group_subgraph). Never called from the update path.
//
// The selection of dppr_topk.hpp leaves, per lane i, the order v_0 .. v_{L-1} and L on the device, and k_cl_rank of
// dppr_cluster.hpp scatters the positions into the rank table (rho_i(w), CL_ABSENT outside the order). Row j of lane i is then the
// multiset {rho_i(w) : w a head of a stored out-edge of v_j, rho_i(w) != CL_ABSENT}, written in ascending order. A sorted multiset
// of integers has one representation, so whichever kernel places a row, and in whatever order it meets the entries, the bytes are
// the same; no output position comes from the return value of an atomic.
//
//   k_sg_count  one wave per (lane, position): the out-row read coalesced 64 entries at a time, one gather of a rank per entry, the
//               matches counted wave-uniformly (popcount of a ballot). A row of more than CL_SPLIT entries is not walked here: the
//               wave queues its chunks on the chunk list of dppr_cluster_plan.hpp (cl_item, direction 0)
//   k_sg_big    one wave per queued chunk, from a fixed grid; its count joins the row's by one integer vector atomic
//   k_sg_scan   one workgroup per lane: exclusive scan of the lane's counts in LDS (cl_block_scan), the entries of the lanes before
//               it summed the same way, row_ptr [k + 1] in absolute indices, the lane's offset and L into the head. The host reads
//               the head once and decides whether the fill runs
//   k_sg_fill   one wave per (lane, position). A row of at most wave_max matches (and at most CL_SPLIT entries) is placed here:
//               the matched positions are compacted into the wave's 1 KiB of LDS in entry order (ballot + mbcnt), and entry t goes
//               to the slot that is the number of smaller (position, t) pairs. Any other row with a match is queued for k_sg_long
//   k_sg_long   one workgroup per queued row, from a fixed grid: a histogram over the k positions in LDS (32 KiB; LDS integer
//               adds, a sum), an exclusive scan of it, and every position emitted as often as it was counted
// Every result is written with ordinary vector stores.
#pragma once

#include "dppr_cluster.hpp"
#include "dppr_subgraph_plan.hpp"

namespace dppr {

struct SgCtl {          // zeroed per call
    unsigned n_items;   // chunk items queued by k_sg_count
    unsigned n_long;    // rows queued by k_sg_fill
    unsigned pad[2];
};
static_assert(sizeof(SgCtl) == 4 * sizeof(int), "sg_work_elems counts four control words");

// entries [lo, hi) of an out-row: how many heads lie in the lane's order
__device__ __forceinline__ int sg_walk(const ClGraph &g, const unsigned short *__restrict__ rank, int stride, int lane, int lo, int hi) {
    int a = 0;
    for (int e0 = lo; e0 < hi; e0 += WAVE) {
        const int e = e0 + lane_id();
        int rho = CL_ABSENT;
        if (e < hi) rho = cl_rank_of(g, rank, stride, lane, ld_stream(g.out_col + e));
        a += __popcll(__ballot(rho != CL_ABSENT));
    }
    return a;
}

// grid: ceil(n * k / 4), one wave per (lane, position). m [n][k]: matched entries of every row (0 past the count)
__global__ __launch_bounds__(CL_BLOCK) void k_sg_count(ClGraph g, const int *__restrict__ ext2int, const int *__restrict__ cnt,
                                                       const int *__restrict__ ids, int n, int k, int stride,
                                                       const unsigned short *__restrict__ rank, int *__restrict__ m, SgCtl *__restrict__ ctl,
                                                       unsigned long long *__restrict__ list, unsigned list_cap) {
    const int pos = blockIdx.x * CL_WAVES + wave_id();
    if (pos >= n * k) return;
    const int lane = pos / k, j = pos - lane * k;
    int c = 0;
    if (j < min(cnt[lane], k)) {
        const int u = __builtin_amdgcn_readfirstlane(ext2int[ids[pos]]);
        if (u >= 0) { // (a vertex of the order has a row of the state: always)
            const int o0 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u]), o1 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u + 1]);
            if (o1 - o0 > CL_SPLIT) {
                const unsigned queued = (unsigned)cl_chunks(o1 - o0);
                unsigned base = 0;
                if (lane_id() == 0) base = atomicAdd(&ctl->n_items, queued);
                base = __builtin_amdgcn_readfirstlane(base);
                for (unsigned q = lane_id(); q < queued; q += WAVE)
                    if (base + q < list_cap) list[base + q] = cl_item((unsigned)pos, 0u, q); // (cl_list_cap bounds what a call can queue)
            } else {
                c = sg_walk(g, rank, stride, lane, o0, o1);
            }
        }
    }
    if (lane_id() == 0) m[pos] = c;
}

// fixed grid, one wave per queued chunk
__global__ __launch_bounds__(CL_BLOCK) void k_sg_big(ClGraph g, const int *__restrict__ ext2int, const int *__restrict__ ids, int k, int stride,
                                                     const unsigned short *__restrict__ rank, int *__restrict__ m,
                                                     const SgCtl *__restrict__ ctl, const unsigned long long *__restrict__ list,
                                                     unsigned list_cap) {
    const unsigned n_items = min(ctl->n_items, list_cap);
    for (unsigned t = blockIdx.x * CL_WAVES + wave_id(); t < n_items; t += gridDim.x * CL_WAVES) {
        const unsigned long long it = list[t];
        const int pos = (int)cl_item_pos(it);
        const int lane = pos / k;
        const int u = __builtin_amdgcn_readfirstlane(ext2int[ids[pos]]);
        const int r0 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u]), r1 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u + 1]);
        const long long lo = (long long)r0 + (long long)cl_item_chunk(it) * CL_SPLIT;
        const int hi = (int)min((long long)r1, lo + CL_SPLIT);
        const int c = lo < hi ? sg_walk(g, rank, stride, lane, (int)lo, hi) : 0;
        if (lane_id() == 0 && c) atomicAdd(&m[pos], c);
    }
}

// grid: n, one workgroup per lane. row_ptr [n][k + 1]
__global__ __launch_bounds__(CL_SCAN_BLOCK) void k_sg_scan(const int *__restrict__ cnt, const int *__restrict__ m, int n, int k,
                                                           SgHead *__restrict__ head, long long *__restrict__ row_ptr) {
    __shared__ long long s_w[CL_SCAN_BLOCK / WAVE];
    __shared__ long long s_tot[2];
    const int lane = blockIdx.x, tid = threadIdx.x;
    const int j0 = tid * CL_PER_THREAD;
    long long v[CL_PER_THREAD];
    long long own = 0, prior = 0; // this thread's positions: of this lane, and of every lane before it
#pragma unroll
    for (int t = 0; t < CL_PER_THREAD; ++t) {
        const int j = j0 + t;
        v[t] = own; // (exclusive inside the thread)
        if (j < k) own += (long long)m[(size_t)lane * k + j];
    }
    for (int l = 0; l < lane; ++l)
#pragma unroll
        for (int t = 0; t < CL_PER_THREAD; ++t)
            if (j0 + t < k) prior += (long long)m[(size_t)l * k + j0 + t];
    const long long own_incl = cl_block_scan(own, s_w), prior_incl = cl_block_scan(prior, s_w);
    if (tid == CL_SCAN_BLOCK - 1) {
        s_tot[0] = own_incl;
        s_tot[1] = prior_incl;
    }
    __syncthreads();
    const long long total = s_tot[0], off = s_tot[1], before = own_incl - own;
    long long *rp = row_ptr + (size_t)lane * ((size_t)k + 1);
#pragma unroll
    for (int t = 0; t < CL_PER_THREAD; ++t)
        if (j0 + t < k) rp[j0 + t] = off + before + v[t]; // (a position past the count matched nothing: it holds the lane's end)
    if (tid == 0) {
        rp[k] = off + total;
        head->offsets[lane] = off;
        head->count[lane] = min(cnt[lane], k);
        if (lane == n - 1) {
            for (int i = n; i <= Q_LANES; ++i) head->offsets[i] = off + total;
            for (int i = n; i < Q_LANES; ++i) head->count[i] = 0;
        }
    }
}

// grid: ceil(n * k / 4), one wave per (lane, position)
__global__ __launch_bounds__(CL_BLOCK) void k_sg_fill(ClGraph g, const int *__restrict__ ext2int, const int *__restrict__ cnt,
                                                      const int *__restrict__ ids, int n, int k, int stride,
                                                      const unsigned short *__restrict__ rank, const long long *__restrict__ row_ptr,
                                                      int wave_max, int *__restrict__ col, SgCtl *__restrict__ ctl, int *__restrict__ long_list) {
    __shared__ int s_key[CL_WAVES][SG_WAVE_CAP];
    const int pos = blockIdx.x * CL_WAVES + wave_id();
    if (pos >= n * k) return;
    const int lane = pos / k, j = pos - lane * k;
    if (j >= min(cnt[lane], k)) return;
    const long long *rp = row_ptr + (size_t)lane * ((size_t)k + 1) + j;
    const long long base = rp[0];
    const int mm = (int)(rp[1] - base);
    if (mm <= 0) return;
    const int u = __builtin_amdgcn_readfirstlane(ext2int[ids[pos]]);
    const int o0 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u]), o1 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u + 1]);
    if (sg_row_is_long(o1 - o0, mm, min(wave_max, SG_WAVE_CAP))) {
        if (lane_id() == 0) long_list[atomicAdd(&ctl->n_long, 1u)] = pos; // (at most one per position: the list holds n * k)
        return;
    }
    int *key = s_key[wave_id()];
    int filled = 0;
    for (int e0 = o0; e0 < o1; e0 += WAVE) {
        const int e = e0 + lane_id();
        int rho = CL_ABSENT;
        if (e < o1) rho = cl_rank_of(g, rank, stride, lane, ld_stream(g.out_col + e));
        const bool hit = rho != CL_ABSENT;
        const uint64_t b = __ballot(hit);
        const int at = filled + mbcnt(b);
        if (hit && at < SG_WAVE_CAP) key[at] = rho;
        filled += __popcll(b);
    }
    __builtin_amdgcn_wave_barrier();
    const int have = min(filled, mm); // (the count pass saw the same row: equal)
    for (int t = lane_id(); t < have; t += WAVE) {
        const int kt = key[t];
        int r = 0;
        for (int q = 0; q < have; ++q) {
            const int kq = key[q];
            r += (kq < kt || (kq == kt && q < t)) ? 1 : 0;
        }
        col[base + r] = kt;
    }
}

// fixed grid, one workgroup per queued row
__global__ __launch_bounds__(SG_LONG_BLOCK) void k_sg_long(ClGraph g, const int *__restrict__ ext2int, const int *__restrict__ ids, int k,
                                                           int stride, const unsigned short *__restrict__ rank,
                                                           const long long *__restrict__ row_ptr, int *__restrict__ col,
                                                           const SgCtl *__restrict__ ctl, const int *__restrict__ long_list, unsigned long_cap) {
    __shared__ int s_hist[DPPR_SUBGRAPH_MAX];
    __shared__ long long s_w[SG_LONG_BLOCK / WAVE];
    const int tid = threadIdx.x;
    const unsigned n_long = min(ctl->n_long, long_cap);
    for (unsigned t = blockIdx.x; t < n_long; t += gridDim.x) {
        const int pos = long_list[t];
        const int lane = pos / k, j = pos - lane * k;
        const int u = ext2int[ids[pos]];
        const int o0 = g.out_row_ptr[u], o1 = g.out_row_ptr[u + 1];
        const long long *rp = row_ptr + (size_t)lane * ((size_t)k + 1) + j;
        const long long base = rp[0], end = rp[1];
        for (int b = tid; b < DPPR_SUBGRAPH_MAX; b += SG_LONG_BLOCK) s_hist[b] = 0;
        __syncthreads();
        for (int e = o0 + tid; e < o1; e += SG_LONG_BLOCK) {
            const int rho = cl_rank_of(g, rank, stride, lane, ld_stream(g.out_col + e));
            if (rho < k) atomicAdd(&s_hist[rho], 1); // (CL_ABSENT is above every k)
        }
        __syncthreads();
        const int b0 = tid * SG_PER_THREAD;
        int c[SG_PER_THREAD];
        long long tot = 0;
#pragma unroll
        for (int q = 0; q < SG_PER_THREAD; ++q) {
            c[q] = s_hist[b0 + q];
            tot += c[q];
        }
        long long w = base + cl_block_scan(tot, s_w) - tot;
#pragma unroll
        for (int q = 0; q < SG_PER_THREAD; ++q)
            for (int x = 0; x < c[q] && w < end; ++x) col[w++] = b0 + q; // (the count pass saw the same row: w ends at `end`)
        __syncthreads(); // (the histogram is zeroed again for the next row)
    }
}

} // namespace dppr
