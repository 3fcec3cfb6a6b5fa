// dppr_position.hpp -- positions of given vertices in a lane's order (dppr_position_at / dppr_group_position_at): the stage
// between the scratch state of the ranked family (dppr_rank.hpp: k_rk_scores) and the scores at the queried ids (k_rk_score_at),
// which counts per (query, lane) the rows of the scratch that precede it. Never called from the update path.
//
// KEYS. A row qualifies iff score > min_score (min_score >= 0; false for a NaN), so a qualifying score is a positive double or
// +inf and its bit pattern orders it. pos_key = ~bits: ascending keys are descending scores, and the order of dppr_topk_ranked is
// (key ascending, external id ascending). Only scores that passed the filter are ever turned into a key: before it the raw
// patterns do NOT order (a negative or a NaN pattern lies above every positive one). ~bits of a positive double is never all
// ones, so POS_KEY_OUT marks a query that does not qualify and orders it last.
//
// SHAPE (dppr_position_plan.hpp has the arithmetic).
//   k_pos_order   grid (pieces of 256 queries, lanes): the lane's m query keys and ids in LDS, one query per thread, its place in
//                 the lane's order by RANK -- the number of queries before it under (key, id, place in `ids`), a total order, so
//                 the places are a permutation and duplicates of an id stand beside each other. Writes key and place at that
//                 position.
//   k_pos_count   THE HOT KERNEL. grid (x, lane blocks, passes). A workgroup holds `tile` consecutive positions of the order of
//                 each of its `lanes` lanes in LDS (key, id, a histogram slot) and streams the scratch rows: thread t serves lane
//                 t % lanes of row t / lanes of a step, so its lane never changes. Per entry: the filter, a count in a register
//                 (pass 0 only), then the first position of the tile that the entry PRECEDES -- strictly before it in
//                 (key, id); an entry equal in both is that vertex itself -- by binary search, and one LDS add to that slot.
//                 Entries that precede nothing of the tile add nothing. A workgroup flushes its non-zero slots and its counts
//                 once, with 32-bit integer atomics: the sums do not depend on the order of arrival.
//   k_pos_finish  one workgroup per lane: an inclusive sum over the slots of every tile (an entry that precedes a position
//                 precedes every later one, and one that precedes a position of an earlier tile landed in slot 0 of this one:
//                 every tile is complete in itself), un-permuted into pos[place][lane], -1 where the query does not qualify;
//                 the lane's count beside it. One result block.
// DESIGN.md section 9m has the byte counts of this shape.
#pragma once

#include "dppr_common.hpp"
#include "dppr_position_plan.hpp"

namespace dppr {

static_assert(POS_BLOCK == 16 * WAVE && POS_ORDER_BLOCK == 4 * WAVE && Q_LANES == GS_MAX, "dppr_position_plan.hpp restates the wave and the lanes");

constexpr unsigned long long POS_KEY_OUT = ~0ull; // a query that does not qualify: after every key

__device__ __forceinline__ unsigned long long pos_key(double score) { return ~(unsigned long long)__double_as_longlong(score); }
// (ka, ia) strictly before (kb, ib) in the order of dppr_topk_ranked
__device__ __forceinline__ bool pos_before(unsigned long long ka, int ia, unsigned long long kb, int ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// qs [m][n]: the scores at the queried ids (k_rk_score_at). key, place: [n][m], by position in the lane's order.
__global__ __launch_bounds__(POS_ORDER_BLOCK) void k_pos_order(const double *__restrict__ qs, const int *__restrict__ ids, int m, int n,
                                                               double min_score, unsigned long long *__restrict__ key,
                                                               int *__restrict__ place) {
    __shared__ unsigned long long s_key[DPPR_POSITION_MAX];
    __shared__ int s_id[DPPR_POSITION_MAX];
    const int lane = blockIdx.y;
    for (int j = threadIdx.x; j < m; j += POS_ORDER_BLOCK) {
        const double x = qs[(size_t)j * n + lane];
        s_key[j] = x > min_score ? pos_key(x) : POS_KEY_OUT;
        s_id[j] = ids[j];
    }
    __syncthreads();
    const int j = blockIdx.x * POS_ORDER_BLOCK + threadIdx.x;
    if (j >= m) return;
    const unsigned long long k = s_key[j];
    const int id = s_id[j];
    int rank = 0;
    for (int o = 0; o < m; ++o) { // (every thread reads the same word: a broadcast)
        const unsigned long long ko = s_key[o];
        const int io = s_id[o];
        rank += (pos_before(ko, io, k, id) || (ko == k && io == id && o < j)) ? 1 : 0;
    }
    key[(size_t)lane * m + rank] = k;
    place[(size_t)lane * m + rank] = j;
}

// score [rows][n], ext [rows]: the scratch state. key / place as k_pos_order wrote them, ids the queried ids.
// slots [n][m + 1], zeroed by the caller: per position the entries whose first preceded position of its tile it is; [m] the count.
__global__ __launch_bounds__(POS_BLOCK) void k_pos_count(const double *__restrict__ score, const int *__restrict__ ext, int rows, int n,
                                                         double min_score, const unsigned long long *__restrict__ key,
                                                         const int *__restrict__ place, const int *__restrict__ ids, int m, int tile,
                                                         int lanes, unsigned *__restrict__ slots) {
    extern __shared__ unsigned long long s_pos[]; // [lanes][tile] keys, then ids, then slots, then Q_LANES counts
    unsigned long long *s_key = s_pos;
    int *s_id = reinterpret_cast<int *>(s_key + (size_t)lanes * tile);
    unsigned *s_hist = reinterpret_cast<unsigned *>(s_id + (size_t)lanes * tile);
    unsigned *s_cnt = s_hist + (size_t)lanes * tile;
    const int l0 = blockIdx.y * lanes, nl = min(lanes, n - l0);
    const int q0 = blockIdx.z * tile, tc = max(min(tile, m - q0), 0);
    for (int o = threadIdx.x; o < nl * tc; o += POS_BLOCK) {
        const int j = o / tc, t = o % tc;
        const size_t at = (size_t)(l0 + j) * m + q0 + t;
        s_key[j * tile + t] = key[at];
        s_id[j * tile + t] = ids[place[at]];
        s_hist[j * tile + t] = 0u;
    }
    if (threadIdx.x < Q_LANES) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int per = POS_BLOCK / lanes;
    const int j = threadIdx.x % lanes, rs = threadIdx.x / lanes;
    unsigned cnt = 0;
    if (j < nl && rs < per) {
        const unsigned long long *kj = s_key + j * tile;
        const int *ij = s_id + j * tile;
        for (long long r = (long long)blockIdx.x * per + rs; r < rows; r += (long long)gridDim.x * per) {
            const double x = score[(size_t)r * n + l0 + j];
            if (!(x > min_score)) continue; // (false for a NaN: nothing below sees a pattern that does not order)
            ++cnt;
            const unsigned long long k = pos_key(x);
            const int u = ext[r];
            int lo = 0, hi = tc;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pos_before(k, u, kj[mid], ij[mid])) hi = mid;
                else lo = mid + 1;
            }
            if (lo < tc) atomicAdd(&s_hist[j * tile + lo], 1u);
        }
        if (blockIdx.z == 0 && cnt) atomicAdd(&s_cnt[j], cnt);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < nl * tc; o += POS_BLOCK) {
        const int jj = o / tc, t = o % tc;
        const unsigned h = s_hist[jj * tile + t];
        if (h) atomicAdd(&slots[(size_t)(l0 + jj) * (m + 1) + q0 + t], h);
    }
    if (blockIdx.z == 0 && threadIdx.x < nl && s_cnt[threadIdx.x]) atomicAdd(&slots[(size_t)(l0 + threadIdx.x) * (m + 1) + m], s_cnt[threadIdx.x]);
}

// res_cnt [16], res_pos [m][n]
__global__ __launch_bounds__(POS_BLOCK) void k_pos_finish(const unsigned *__restrict__ slots, const unsigned long long *__restrict__ key,
                                                          const int *__restrict__ place, int m, int n, int tile, int *__restrict__ res_cnt,
                                                          int *__restrict__ res_pos) {
    __shared__ unsigned s_sum[POS_BLOCK];
    constexpr int PER = POS_LDS_QUERIES / POS_BLOCK; // consecutive positions of a tile a thread owns
    const int lane = blockIdx.x;
    const unsigned *sl = slots + (size_t)lane * (m + 1);
    if (threadIdx.x == 0) res_cnt[lane] = (int)sl[m];
    for (int q0 = 0; q0 < m; q0 += tile) {
        const int tc = min(tile, m - q0);
        unsigned v[PER], tot = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int t = threadIdx.x * PER + i;
            v[i] = t < tc ? sl[q0 + t] : 0u;
            tot += v[i];
        }
        s_sum[threadIdx.x] = tot;
        __syncthreads();
        for (int off = 1; off < POS_BLOCK; off <<= 1) {
            const unsigned a = threadIdx.x >= off ? s_sum[threadIdx.x - off] : 0u;
            __syncthreads();
            s_sum[threadIdx.x] += a;
            __syncthreads();
        }
        unsigned run = s_sum[threadIdx.x] - tot;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int t = threadIdx.x * PER + i;
            run += v[i];
            if (t < tc) {
                const size_t at = (size_t)lane * m + q0 + t;
                res_pos[(size_t)place[at] * n + lane] = key[at] == POS_KEY_OUT ? -1 : (int)run;
            }
        }
        __syncthreads(); // (s_sum is written again by the next tile)
    }
}

} // namespace dppr
