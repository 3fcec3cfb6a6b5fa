// dppr_patch.hpp -- the step from one thresholded state to the next: what to write into a replica of {p > min_p} and what to
// remove from it (dppr_patch / dppr_group_patch), against the mark of dppr_changes.hpp. Never called from the update path.
//
// Every kernel walks the EXTERNAL ids in tiles of EX_TILE, one id per thread, as dppr_export.hpp does, so id order is the order
// of the threads and no output position comes from an atomic:
//   k_pt_classify  row = ext2int[ext]; the gathered gw-wide p row and the contiguous mark row of the id are loaded in ONE iteration
//                  (both in flight together, as in k_ch_delta; 16-byte loads where gw is even, 8-byte loads on a slot). A vertex
//                  without an id has p = 0.0. Per lane: now = p > min_p, then = mark > min_p, d = __dsub_rn(p, mark);
//                  UPSERT = now && (!then || |d| > min_delta), DELETE = then && !now. One 32-bit word per id (upserts low, deletes
//                  high) and the tile's counts of both kinds per lane: a ballot and a popcount per lane, kind and wave, the waves
//                  combined in LDS.
//   k_pt_scan      ONE workgroup, wave i = lane i, both kinds in turn (the sibling of k_ex_scan, which stays as it is: it knows
//                  one kind and one cap): the totals, twice n + 1 offsets, the exclusive scans of the tile counts into 64-bit
//                  bases; go = both totals inside their caps, decided here.
//   k_pt_fill      returns at once unless go. Streams the mask words (4-byte reads); a tile of zero words costs those and a
//                  barrier, except under REMARK_ALL, which visits every id. p is gathered again by the threads that emit an
//                  upsert (and, under REMARK_EMITTED, a delete: the mark takes its p); every entry goes to base[tile][kind][lane]
//                  + (entries of the preceding waves, LDS) + mbcnt of the lane's ballot. The re-mark stores p into the mark row
//                  of the thread's own id: whole rows under REMARK_ALL (0.0 for a vertex without an id, as k_ch_mark), the emitted
//                  lanes alone under REMARK_EMITTED.
// Every store is an ordinary vector store.
#pragma once

#include "dppr_common.hpp"
#include "dppr_export.hpp"
#include "dppr_patch_plan.hpp"

namespace dppr {

__device__ __forceinline__ void pt_classify_one(double p, double m, double min_p, double min_delta, int l, unsigned &word) {
    const bool now = p > min_p, then = m > min_p;
    const double d = __dsub_rn(p, m);
    word |= (unsigned)(now && (!then || fabs(d) > min_delta)) << l;
    word |= (unsigned)(then && !now) << (16 + l);
}

// mark: [V][gw]. mask: [V] (every id is written), cnt: [tiles][2][n]
__global__ __launch_bounds__(EX_TILE) void k_pt_classify(const double *__restrict__ p, int gw, int n, const int *__restrict__ ext2int,
                                                         int V, const double *__restrict__ mark, double min_p, double min_delta,
                                                         unsigned *__restrict__ mask, int *__restrict__ cnt) {
    __shared__ int s_cnt[EX_WAVES][2 * PT_LANES];
    const int tiles = (V + EX_TILE - 1) / EX_TILE;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ext = tile * EX_TILE + (int)threadIdx.x;
        unsigned m = 0;
        if (ext < V) {
            const int row = ext2int[ext];
            const double *mr = mark + (size_t)ext * gw;
            const double *pr = p + (size_t)(row >= 0 ? row : 0) * gw;
            if (gw & 1) { // a single-source slot: rows of one double
                for (int l = 0; l < n; ++l) {
                    const double vm = mr[l];
                    const double vp = row >= 0 ? pr[l] : 0.0;
                    pt_classify_one(vp, vm, min_p, min_delta, l, m);
                }
            } else {
                for (int h = 0; 2 * h < n; ++h) {
                    const double2 vm = *reinterpret_cast<const double2 *>(mr + 2 * h);
                    double2 vp = make_double2(0.0, 0.0);
                    if (row >= 0) vp = *reinterpret_cast<const double2 *>(pr + 2 * h);
                    pt_classify_one(vp.x, vm.x, min_p, min_delta, 2 * h, m);
                    if (2 * h + 1 < n) pt_classify_one(vp.y, vm.y, min_p, min_delta, 2 * h + 1, m);
                }
            }
            mask[ext] = m;
        }
        for (int l = 0; l < n; ++l) {
            const uint64_t bu = __ballot((m >> l) & 1u), bd = __ballot((m >> (16 + l)) & 1u);
            if (lane_id() == 0) {
                s_cnt[wave_id()][l] = __popcll(bu);
                s_cnt[wave_id()][n + l] = __popcll(bd);
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * n) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < EX_WAVES; ++w) c += s_cnt[w][threadIdx.x];
            cnt[(size_t)tile * 2 * n + threadIdx.x] = c;
        }
        __syncthreads(); // (the counts are read before the next tile overwrites them)
    }
}

// One workgroup of PT_LANES waves. head: both sets of offsets, go, written; base: [tiles][2][n].
__global__ __launch_bounds__(PT_LANES * WAVE) void k_pt_scan(const int *__restrict__ cnt, int n, int tiles, long long cap_up,
                                                             long long cap_del, long long *__restrict__ base,
                                                             PtHead *__restrict__ head) {
    __shared__ long long s_total[2][PT_LANES], s_off[2][PT_LANES + 1];
    const int l = wave_id(), li = lane_id();
    if (l < n) {
        for (int k = 0; k < 2; ++k) {
            long long sum = 0;
            for (int t = li; t < tiles; t += WAVE) sum += cnt[(size_t)t * 2 * n + k * n + l];
            for (int d = WAVE / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
            if (li == 0) s_total[k][l] = sum;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tot[2];
        for (int k = 0; k < 2; ++k) {
            long long *off = k ? head->del_offsets : head->up_offsets;
            long long o = 0;
            for (int i = 0; i <= PT_LANES; ++i) {
                s_off[k][i] = o;
                off[i] = o;
                if (i < n) o += s_total[k][i];
            }
            tot[k] = o;
        }
        const int go = tot[0] <= cap_up && tot[1] <= cap_del ? 1 : 0;
        head->go = go;
        head->written = go;
    }
    __syncthreads();
    if (l < n) {
        for (int k = 0; k < 2; ++k) {
            long long carry = s_off[k][l];
            for (int t0 = 0; t0 < tiles; t0 += WAVE) { // (a tile holds at most EX_TILE ids: 64 of them sum far inside an int)
                const int t = t0 + li;
                const int c = t < tiles ? cnt[(size_t)t * 2 * n + k * n + l] : 0;
                const int inc = wave_inclusive_scan(c);
                if (t < tiles) base[(size_t)t * 2 * n + k * n + l] = carry + (inc - c);
                carry += __builtin_amdgcn_readlane(inc, WAVE - 1);
            }
        }
    }
}

// up_ids / up_p: head->up_offsets[n] entries, del_ids: head->del_offsets[n] entries, written only if head->go (all three may be
// NULL where their total is 0). remark: DPPR_PATCH_*; the mark row of an id is stored by the thread of that id alone.
__global__ __launch_bounds__(EX_TILE) void k_pt_fill(const double *__restrict__ p, int gw, int n, const int *__restrict__ ext2int, int V,
                                                     double *__restrict__ mark, const unsigned *__restrict__ mask,
                                                     const long long *__restrict__ base, const PtHead *__restrict__ head, int remark,
                                                     int *__restrict__ up_ids, double *__restrict__ up_p, int *__restrict__ del_ids) {
    __shared__ int s_cnt[EX_WAVES][2 * PT_LANES];
    __shared__ long long s_base[2 * PT_LANES];
    if (!head->go) return;
    const int tiles = (V + EX_TILE - 1) / EX_TILE;
    const int w = wave_id();
    const bool all = remark == DPPR_PATCH_REMARK_ALL, emitted = remark == DPPR_PATCH_REMARK_EMITTED;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ext = tile * EX_TILE + (int)threadIdx.x;
        const unsigned m = ext < V ? mask[ext] : 0u;
        const bool any = __syncthreads_or((int)m); // (the same in every thread of the workgroup)
        if (!any && !all) continue;
        const unsigned mu = m & 0xffffu, md = m >> 16;
        if (any) {
            for (int l = 0; l < n; ++l) {
                const uint64_t bu = __ballot((mu >> l) & 1u), bd = __ballot((md >> l) & 1u);
                if (lane_id() == 0) {
                    s_cnt[w][l] = __popcll(bu);
                    s_cnt[w][n + l] = __popcll(bd);
                }
            }
            if ((int)threadIdx.x < 2 * n) s_base[threadIdx.x] = base[(size_t)tile * 2 * n + threadIdx.x];
            __syncthreads();
        }
        const unsigned need_p = all ? 0xffffu : (mu | (emitted ? md : 0u)); // the lanes whose p this thread delivers or marks
        const int row = ext < V && need_p ? ext2int[ext] : -1;
        for (int h = 0; 2 * h < gw; ++h) {
            const int l0 = 2 * h, l1 = 2 * h + 1;
            const bool u0 = (mu >> l0) & 1u, u1 = (mu >> l1) & 1u, d0 = (md >> l0) & 1u, d1 = (md >> l1) & 1u;
            const uint64_t bu0 = __ballot(u0), bu1 = __ballot(u1), bd0 = __ballot(d0), bd1 = __ballot(d1);
            if (!all && (bu0 | bu1 | bd0 | bd1) == 0) continue; // (wave-uniform)
            if (ext < V && (all | u0 | u1 | d0 | d1)) {
                double2 vp = make_double2(0.0, 0.0);
                if (row >= 0 && ((need_p >> l0) & 3u)) {
                    const size_t at = (size_t)row * gw + l0;
                    if (gw & 1) vp.x = p[at]; // a single-source slot: rows of one double
                    else vp = *reinterpret_cast<const double2 *>(p + at);
                }
                double *mr = mark + (size_t)ext * gw;
                if (all) {
                    if (gw & 1) mr[l0] = vp.x;
                    else *reinterpret_cast<double2 *>(mr + l0) = vp;
                } else if (emitted) {
                    if (u0 | d0) mr[l0] = vp.x;
                    if (u1 | d1) mr[l1] = vp.y;
                }
                if (u0) {
                    long long pos = s_base[l0] + mbcnt(bu0);
                    for (int k = 0; k < w; ++k) pos += s_cnt[k][l0];
                    up_ids[pos] = ext;
                    up_p[pos] = vp.x;
                }
                if (u1) {
                    long long pos = s_base[l1] + mbcnt(bu1);
                    for (int k = 0; k < w; ++k) pos += s_cnt[k][l1];
                    up_ids[pos] = ext;
                    up_p[pos] = vp.y;
                }
                if (d0) {
                    long long pos = s_base[n + l0] + mbcnt(bd0);
                    for (int k = 0; k < w; ++k) pos += s_cnt[k][n + l0];
                    del_ids[pos] = ext;
                }
                if (d1) {
                    long long pos = s_base[n + l1] + mbcnt(bd1);
                    for (int k = 0; k < w; ++k) pos += s_cnt[k][n + l1];
                    del_ids[pos] = ext;
                }
            }
        }
        if (any) __syncthreads(); // (the counts and bases are read before the next tile overwrites them)
    }
}

} // namespace dppr
