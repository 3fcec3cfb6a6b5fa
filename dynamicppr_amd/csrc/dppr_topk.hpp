// dppr_topk.hpp -- queries of a PPR state on the device: top-k per source (dppr_topk, dppr_group_topk) and point reads
// (dppr_read_at, dppr_group_read_at). Never called from the update path.
//
// One selection serves both layouts: a single-source slot is a group of one source with rows one double wide. A
// state is p[row * gw + lane], lane < n (n <= 16; lanes n .. gw-1 are padding and never looked at), and only the rows
// that hold a vertex are scanned: the live zone [0, n_int) and the parked zone [V - n_parked, V) (dppr_idspace.hpp).
//
// ORDER. A candidate has p > min_p >= 0, so its bit pattern is a positive double and monotone as a uint64. The result
// order (p descending, external id ascending) is the descending order of the 96-bit composite
//     U = key(p) : ~ext    (hi 64 bits : lo 32 bits)
// which is unique per lane. The k largest U are found by a radix select on U, then ordered by rank.
//
//   pass 1   k_tk_hist1     full stream of the occupied rows: per lane, a histogram of the exponent digit (key bits 62..52,
//                           2048 bins; the sign bit is 0), privatised in LDS, one global add per non-empty bin and block
//   select   k_tk_select1   per lane: the boundary bin b1 where the count from the top reaches k. Everything above it is in
//                           the result; if the whole bin fits too (or fewer than k qualify) the lane is done
//   pass 2   k_tk_compact   full stream again: entries above b1 (or at it, for a done lane) go to the lane's result list,
//                           entries inside an open b1 to its candidate list (row index only)
//   refine   k_tk_hist2 / k_tk_select2, 7 rounds of 12 bits over the candidate list only (84 = 52 key + 32 id bits):
//                           each round fixes one more digit of the threshold T; a lane is done once its bucket fits whole
//   take     k_tk_take      candidates with U >= T join the result list (exactly what was still needed)
//   order    k_tk_rank      rank of each result entry = number of entries with a larger U; entries past the count: id -1,
//                           value 0.0. The counts, ids, p and r of all lanes lie in one buffer: one copy to the host
//
// The full state is read twice whatever k and n are; the refinement rounds read the candidate list (the boundary bin:
// ~k to a few k entries on PPR states) and are no-ops for lanes that are done. No step reads back to the host.
// Every result is written with ordinary vector stores; counters are global / LDS vector atomics.
#pragma once

#include "dppr_common.hpp"

namespace dppr {

constexpr int TK_BINS1 = 2048;      // pass-1 digit: the exponent (key bits 62..52)
constexpr int TK_DIGIT = 12;        // refinement digit
constexpr int TK_BINS2 = 1 << TK_DIGIT;
constexpr int TK_ROUNDS = 7;        // 84 bits below the exponent: key bits 51..0, then the 32 bits of ~ext
constexpr int TK_SHIFT1 = 84;       // position of the pass-1 digit in U
constexpr int TK_BLOCK = 1024;      // streaming passes: one workgroup per CU holds n x 8 KiB of histogram
constexpr int TK_ROWS = 512;        // rows per chunk of a streaming pass (<= 8 entries per thread)
constexpr int TK_PER_THREAD = TK_ROWS * 16 / TK_BLOCK;

struct TkLane {               // per-lane control word of a selection (zeroed per call)
    unsigned long long t_hi;  // threshold T: U >= T is in the result once the lane is done
    unsigned t_lo;
    int b1;                   // pass-1 boundary bin
    int done;                 // 1: the bucket at the current level is taken whole
    int need;                 // entries still to take from the current bucket
    int n_out, n_cand;        // lengths of the result and the candidate list
};

struct TkState {             // the state being queried
    const double *p, *r;
    int gw, n;               // row width in doubles, lanes that hold a source
    int n_int, lo_parked;    // live zone [0, n_int), parked zone [lo_parked, lo_parked + rows - n_int)
    int rows;                // n_int + n_parked
};

__device__ __forceinline__ int tk_row(const TkState &st, int q) { return q < st.n_int ? q : st.lo_parked + (q - st.n_int); }
__device__ __forceinline__ unsigned long long tk_key(double v) { return (unsigned long long)__double_as_longlong(v); }

// ---- the tile of the kernels that fill a scratch state (k_wq_scores, k_ch_delta, k_rk_scores) ------------------------------
// Such a kernel streams the occupied rows once, TK_TILE_ROWS rows per step and workgroup of TK_TILE_BLOCK threads, and writes a
// COMPACTED state (row c = 0 .. rows - 1, no parked zone) with the external id of every row beside it, over which the selection
// below then runs as it is. A tile of p is staged in LDS rows padded by one double: the threads of a wave that then work on one
// output each read rows 17 (9, 5, ..) doubles apart, which the 64 banks serve without conflict, and the threads of one row read
// the same address (a broadcast).
constexpr int TK_TILE_ROWS = 128;                   // rows per tile: 128 x 17 doubles of LDS (17 KiB) per staged plane
constexpr int TK_TILE_BLOCK = 256;
constexpr int TK_TILE_LDS_ROW = 16 + 1;             // widest padded row (16 lanes: GS_MAX of dppr_multi.hpp)

// Rows [c0, c0 + cnt) of st.p into s_p (row rl at s_p + rl * (gw + 1)) and their external ids into ext_c: 16-byte loads where a
// row is an even number of doubles (every group), 8-byte loads on a single-source slot (gw = 1), consecutive threads at
// consecutive addresses (rows are contiguous inside a zone). per_row(rl, row, ext) runs once per row, by the thread that wrote
// its id. The caller synchronises before it reads s_p.
template <class PerRow>
__device__ __forceinline__ void tk_stage_tile(const TkState &st, const int *__restrict__ i2e, int c0, int cnt, double *s_p,
                                              int *__restrict__ ext_c, PerRow &&per_row) {
    const int ls = st.gw + 1, half = st.gw / 2;
    if (st.gw & 1) {
        for (int j = threadIdx.x; j < cnt * st.gw; j += TK_TILE_BLOCK) {
            const int rl = j / st.gw, h = j % st.gw;
            s_p[rl * ls + h] = st.p[(size_t)tk_row(st, c0 + rl) * st.gw + h];
        }
    } else {
        for (int j = threadIdx.x; j < cnt * half; j += TK_TILE_BLOCK) {
            const int rl = j / half, h = j % half;
            const double2 v = *reinterpret_cast<const double2 *>(st.p + (size_t)tk_row(st, c0 + rl) * st.gw + 2 * h);
            s_p[rl * ls + 2 * h] = v.x;
            s_p[rl * ls + 2 * h + 1] = v.y;
        }
    }
    for (int rl = threadIdx.x; rl < cnt; rl += TK_TILE_BLOCK) {
        const int row = tk_row(st, c0 + rl), ext = i2e[row];
        ext_c[c0 + rl] = ext;
        per_row(rl, row, ext);
    }
}

// digit of U = hi:lo (96 bits) whose lowest bit is bit s
__device__ __forceinline__ int tk_digit(unsigned long long hi, unsigned lo, int s) {
    const unsigned long long w = s >= 32 ? hi >> (s - 32) : (hi << (32 - s)) | ((unsigned long long)lo >> s);
    return (int)(w & (TK_BINS2 - 1));
}
// U and T agree on every bit from q upwards
__device__ __forceinline__ bool tk_same_above(unsigned long long hi, unsigned lo, unsigned long long thi, unsigned tlo, int q) {
    if (q >= 32) return (hi >> (q - 32)) == (thi >> (q - 32));
    return hi == thi && (lo >> q) == (tlo >> q);
}
__device__ __forceinline__ bool tk_at_least(unsigned long long hi, unsigned lo, unsigned long long thi, unsigned tlo) {
    return hi > thi || (hi == thi && lo >= tlo);
}

// One 256-thread block: bins h[0 .. nb) (LDS) read from the top. Returns the bin b where the running count from the top
// first reaches `need` (need >= 1, and the total is >= need), and the count strictly above it.
__device__ void tk_find_bin(const unsigned *h, int nb, int need, int *s_scan, int *out_b, int *out_above) {
    const int tid = threadIdx.x, per = nb / 256;
    const int top = nb - 1 - tid * per; // this thread's bins: top, top-1, .., top-per+1
    int sum = 0;
    for (int j = 0; j < per; ++j) sum += (int)h[top - j];
    s_scan[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) { // inclusive scan, Hillis-Steele
        const int x = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += x;
        __syncthreads();
    }
    int run = s_scan[tid] - sum; // count above this thread's bins
    if (run < need && run + sum >= need) {
        for (int j = 0; j < per; ++j) {
            const int c = (int)h[top - j];
            if (run + c >= need) {
                *out_b = top - j;
                *out_above = run;
                break;
            }
            run += c;
        }
    }
    __syncthreads();
}

// ---- pass 1 -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_BLOCK) void k_tk_hist1(TkState st, double min_p, unsigned *__restrict__ hist) {
    extern __shared__ unsigned s_h1[]; // [n][TK_BINS1]
    const int nh = st.n * TK_BINS1;
    for (int i = threadIdx.x; i < nh; i += TK_BLOCK) s_h1[i] = 0;
    __syncthreads();
    const int per_chunk = TK_ROWS * st.gw;
    const int n_chunks = (st.rows + TK_ROWS - 1) / TK_ROWS;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int q0 = c * TK_ROWS;
        for (int j = threadIdx.x; j < per_chunk; j += TK_BLOCK) {
            const int q = q0 + j / st.gw, lane = j % st.gw;
            if (q >= st.rows || lane >= st.n) continue;
            const double v = st.p[(size_t)tk_row(st, q) * st.gw + lane];
            if (v > min_p) atomicAdd(&s_h1[lane * TK_BINS1 + (int)(tk_key(v) >> 52)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += TK_BLOCK)
        if (s_h1[i]) atomicAdd(&hist[i], s_h1[i]);
}

// ---- select 1: one block per lane --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tk_select1(const unsigned *__restrict__ hist, int k, TkLane *__restrict__ ctl) {
    __shared__ unsigned s_h[TK_BINS1];
    __shared__ int s_scan[256];
    __shared__ int s_b, s_above;
    const int lane = blockIdx.x;
    for (int i = threadIdx.x; i < TK_BINS1; i += 256) s_h[i] = hist[lane * TK_BINS1 + i];
    if (threadIdx.x == 0) s_b = -1, s_above = 0;
    __syncthreads();
    tk_find_bin(s_h, TK_BINS1, k, s_scan, &s_b, &s_above);
    if (threadIdx.x == 0) {
        TkLane &L = ctl[lane];
        if (s_b < 0) { // fewer than k qualify: all of them
            L.b1 = 0;
            L.done = 1;
            L.t_hi = 0;
        } else {
            L.b1 = s_b;
            L.need = k - s_above;
            L.done = (int)s_h[s_b] == L.need ? 1 : 0;
            L.t_hi = (unsigned long long)s_b << (TK_SHIFT1 - 32);
        }
        L.t_lo = 0;
    }
}

// ---- pass 2 -----------------------------------------------------------------------------------------------------
// A chunk's entries are held in registers between the count and the write, so the state is read once: the block
// counts per lane in LDS, reserves one range per lane and list with a global add, then writes.
__global__ __launch_bounds__(TK_BLOCK) void k_tk_compact(TkState st, double min_p, TkLane *__restrict__ ctl, int k,
                                                         unsigned long long *__restrict__ out_key, int *__restrict__ out_row,
                                                         int *__restrict__ cand, int cand_cap) {
    __shared__ int s_b1[16], s_done[16], s_cnt[2][16], s_base[2][16];
    if (threadIdx.x < st.n) {
        s_b1[threadIdx.x] = ctl[threadIdx.x].b1;
        s_done[threadIdx.x] = ctl[threadIdx.x].done;
    }
    const int per_chunk = TK_ROWS * st.gw;
    const int n_chunks = (st.rows + TK_ROWS - 1) / TK_ROWS;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        if (threadIdx.x < 16) s_cnt[0][threadIdx.x] = s_cnt[1][threadIdx.x] = 0;
        __syncthreads();
        const int q0 = c * TK_ROWS;
        unsigned long long key[TK_PER_THREAD];
        int row[TK_PER_THREAD], lane_of[TK_PER_THREAD], slot[TK_PER_THREAD]; // slot: list (bit 30) | index in the block's range
#pragma unroll
        for (int t = 0; t < TK_PER_THREAD; ++t) {
            const int j = threadIdx.x + t * TK_BLOCK;
            slot[t] = -1;
            if (j >= per_chunk) continue;
            const int q = q0 + j / st.gw, lane = j % st.gw;
            if (q >= st.rows || lane >= st.n) continue;
            row[t] = tk_row(st, q);
            lane_of[t] = lane;
            const double v = st.p[(size_t)row[t] * st.gw + lane];
            if (!(v > min_p)) continue;
            key[t] = tk_key(v);
            const int b = (int)(key[t] >> 52), b1 = s_b1[lane];
            const int list = (b > b1 || (b == b1 && s_done[lane])) ? 0 : b == b1 ? 1 : -1;
            if (list >= 0) slot[t] = (list << 30) | atomicAdd(&s_cnt[list][lane], 1);
        }
        __syncthreads();
        if (threadIdx.x < 2 * 16) {
            const int list = threadIdx.x / 16, lane = threadIdx.x % 16;
            const int cnt = s_cnt[list][lane];
            if (lane < st.n && cnt) s_base[list][lane] = atomicAdd(list ? &ctl[lane].n_cand : &ctl[lane].n_out, cnt);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TK_PER_THREAD; ++t) {
            if (slot[t] < 0) continue;
            const int list = slot[t] >> 30, lane = lane_of[t];
            const int at = s_base[list][lane] + (slot[t] & ((1 << 30) - 1));
            if (list == 0) {
                if (at < k) {
                    out_key[(size_t)lane * k + at] = key[t];
                    out_row[(size_t)lane * k + at] = row[t];
                }
            } else if (at < cand_cap) {
                cand[(size_t)lane * cand_cap + at] = row[t];
            }
        }
        __syncthreads(); // (s_cnt / s_base are reused by the next chunk)
    }
}

// ---- refinement over the candidate lists: grid (blocks, n) ------------------------------------------------------
__device__ __forceinline__ void tk_cand_u(const TkState &st, const int *__restrict__ i2e, int row, int lane,
                                          unsigned long long *hi, unsigned *lo) {
    *hi = tk_key(st.p[(size_t)row * st.gw + lane]);
    *lo = ~(unsigned)i2e[row];
}

__global__ __launch_bounds__(256) void k_tk_hist2(TkState st, const int *__restrict__ i2e, const TkLane *__restrict__ ctl,
                                                  const int *__restrict__ cand, int cand_cap, int s,
                                                  unsigned *__restrict__ hist) {
    __shared__ unsigned s_h[TK_BINS2];
    const int lane = blockIdx.y;
    const TkLane L = ctl[lane];
    if (L.done) return;
    const int cnt = min(L.n_cand, cand_cap);
    for (int i = threadIdx.x; i < TK_BINS2; i += 256) s_h[i] = 0;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
        const int row = cand[(size_t)lane * cand_cap + i];
        unsigned long long hi;
        unsigned lo;
        tk_cand_u(st, i2e, row, lane, &hi, &lo);
        if (tk_same_above(hi, lo, L.t_hi, L.t_lo, s + TK_DIGIT)) atomicAdd(&s_h[tk_digit(hi, lo, s)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TK_BINS2; i += 256)
        if (s_h[i]) atomicAdd(&hist[lane * TK_BINS2 + i], s_h[i]);
}

__global__ __launch_bounds__(256) void k_tk_select2(unsigned *__restrict__ hist, int s, TkLane *__restrict__ ctl) {
    __shared__ unsigned s_h[TK_BINS2];
    __shared__ int s_scan[256];
    __shared__ int s_b, s_above;
    const int lane = blockIdx.x;
    if (ctl[lane].done) return;
    for (int i = threadIdx.x; i < TK_BINS2; i += 256) {
        s_h[i] = hist[lane * TK_BINS2 + i];
        hist[lane * TK_BINS2 + i] = 0; // (ready for the next round)
    }
    if (threadIdx.x == 0) s_b = -1, s_above = 0;
    __syncthreads();
    const int need = ctl[lane].need;
    tk_find_bin(s_h, TK_BINS2, need, s_scan, &s_b, &s_above);
    if (threadIdx.x == 0 && s_b >= 0) { // (s_b < 0 cannot happen: the bucket holds more than `need`)
        TkLane &L = ctl[lane];
        const unsigned long long b = (unsigned long long)s_b;
        if (s >= 32) L.t_hi |= b << (s - 32);
        else {
            L.t_lo |= (unsigned)(b << s);
            if (s + TK_DIGIT > 32) L.t_hi |= b >> (32 - s);
        }
        L.need = need - s_above;
        L.done = (int)s_h[s_b] == L.need ? 1 : 0;
    }
}

// candidates at or above the threshold join the result list (lanes that had no candidate list take nothing)
__global__ __launch_bounds__(256) void k_tk_take(TkState st, const int *__restrict__ i2e, TkLane *__restrict__ ctl,
                                                 const int *__restrict__ cand, int cand_cap, int k,
                                                 unsigned long long *__restrict__ out_key, int *__restrict__ out_row) {
    const int lane = blockIdx.y;
    const int cnt = min(ctl[lane].n_cand, cand_cap);
    const unsigned long long thi = ctl[lane].t_hi;
    const unsigned tlo = ctl[lane].t_lo;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
        const int row = cand[(size_t)lane * cand_cap + i];
        unsigned long long hi;
        unsigned lo;
        tk_cand_u(st, i2e, row, lane, &hi, &lo);
        if (!tk_at_least(hi, lo, thi, tlo)) continue;
        const int at = atomicAdd(&ctl[lane].n_out, 1);
        if (at < k) {
            out_key[(size_t)lane * k + at] = hi;
            out_row[(size_t)lane * k + at] = row;
        }
    }
}

// ---- final order: grid (ceil(k / 256), n). res: [16] counts, then ids [n][k], p [n][k], r [n][k] --------------------
__global__ __launch_bounds__(256) void k_tk_rank(TkState st, const int *__restrict__ i2e, const TkLane *__restrict__ ctl, int k,
                                                 const unsigned long long *__restrict__ out_key, const int *__restrict__ out_row,
                                                 int *__restrict__ res_cnt, int *__restrict__ res_id, double *__restrict__ res_p,
                                                 double *__restrict__ res_r) {
    __shared__ unsigned long long s_hi[256];
    __shared__ unsigned s_lo[256];
    const int lane = blockIdx.y;
    const int c = min(ctl[lane].n_out, k);
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long hi = 0;
    unsigned lo = 0;
    int row = 0;
    if (i < c) {
        row = out_row[(size_t)lane * k + i];
        hi = out_key[(size_t)lane * k + i];
        lo = ~(unsigned)i2e[row];
    }
    int rank = 0;
    for (int t0 = 0; t0 < c; t0 += 256) {
        __syncthreads();
        const int j = t0 + threadIdx.x;
        if (j < c) {
            const int rj = out_row[(size_t)lane * k + j];
            s_hi[threadIdx.x] = out_key[(size_t)lane * k + j];
            s_lo[threadIdx.x] = ~(unsigned)i2e[rj];
        }
        __syncthreads();
        const int m = min(256, c - t0);
        if (i < c)
            for (int jj = 0; jj < m; ++jj) {
                const unsigned long long h2 = s_hi[jj];
                rank += (h2 > hi || (h2 == hi && s_lo[jj] > lo)) ? 1 : 0;
            }
    }
    const size_t o = (size_t)lane * k;
    if (i < c) {
        res_id[o + rank] = (int)~lo;
        res_p[o + rank] = __longlong_as_double((long long)hi);
        res_r[o + rank] = st.r[(size_t)row * st.gw + lane];
    } else if (i < k) {
        res_id[o + i] = -1;
        res_p[o + i] = 0.0;
        res_r[o + i] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) res_cnt[lane] = c;
}

// ---- point reads: one thread per (id, lane); out [m][n] ------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_read_at(const double *__restrict__ p, const double *__restrict__ r, int gw, int n,
                                                   const int *__restrict__ ext2int, const int *__restrict__ ids, int m,
                                                   double *__restrict__ out_p, double *__restrict__ out_r) {
    const int64_t total = (int64_t)m * n;
    for (int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * BLOCK) {
        const int i = (int)(t / n), lane = (int)(t % n);
        const int q = ext2int[ids[i]];
        out_p[t] = q >= 0 ? p[(size_t)q * gw + lane] : 0.0;
        out_r[t] = q >= 0 ? r[(size_t)q * gw + lane] : 0.0;
    }
}

} // namespace dppr
