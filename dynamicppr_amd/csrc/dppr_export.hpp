// dppr_export.hpp -- the state leaves the engine: thresholded sparse vectors (dppr_support / dppr_export_sparse and their group
// forms) and dense copies by external id into device memory of the caller (dppr_export_dense_dev). Never called from the update
// path.
//
// SPARSE. Every kernel walks the EXTERNAL ids in tiles of EX_TILE, one id per thread, so id order is the order of the threads
// and no output position comes from an atomic:
//   k_ex_mask   row = ext2int[ext], one gather of the gw-wide p row (16-byte loads where gw is even, 8-byte loads on a slot);
//               a 16-bit mask per id (bit i: p_i > min_p) and the tile's count per lane: a ballot and a popcount per lane
//               and wave, the waves combined in LDS. A vertex without an id, a negative p, -0.0 and NaN fail `>`.
//   k_ex_scan   ONE workgroup, wave i = lane i: the lane's total, the n + 1 offsets, then the exclusive scan of the lane's tile
//               counts into 64-bit bases that start at the lane's offset; go = (offsets[n] <= cap), decided here.
//   k_ex_fill   returns at once unless go. Streams the masks (2-byte reads); a tile of zero masks costs those and a barrier.
//               Otherwise the p (and r) row is gathered again by the threads whose mask is not zero and every qualifying
//               (id, lane) goes to base[tile][lane] + (qualifying ids of the preceding waves, LDS) + mbcnt of the lane's ballot.
// DENSE. k_ex_dense<T, SOURCE_MAJOR>: vertex-major is the pass of k_ch_mark with a conversion (consecutive threads, consecutive
// elements); source-major stages EX_TILE ids x gw lanes in LDS, rows padded by one double (the bank argument of
// dppr_wquery.hpp), and every store instruction writes consecutive addresses of one source's row. f32: __double2float_rn.
// Every store is an ordinary vector store.
#pragma once

#include "dppr_common.hpp"
#include "dppr_export_plan.hpp"

namespace dppr {

constexpr int EX_WAVES = EX_TILE / WAVE;
static_assert(EX_TILE % WAVE == 0 && EX_TILE <= 256, "a tile is a workgroup of whole waves, at most 256 ids");

// mask: [V] (every id is written), cnt: [tiles][n]
__global__ __launch_bounds__(EX_TILE) void k_ex_mask(const double *__restrict__ p, int gw, int n, const int *__restrict__ ext2int,
                                                     int V, double min_p, unsigned short *__restrict__ mask,
                                                     int *__restrict__ cnt) {
    __shared__ int s_cnt[EX_WAVES][EX_LANES];
    const int tiles = (V + EX_TILE - 1) / EX_TILE;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ext = tile * EX_TILE + (int)threadIdx.x;
        const int row = ext < V ? ext2int[ext] : -1;
        unsigned m = 0;
        if (row >= 0) {
            const double *pr = p + (size_t)row * gw;
            if (gw & 1) { // a single-source slot: rows of one double
                for (int l = 0; l < n; ++l) m |= (unsigned)(pr[l] > min_p) << l;
            } else {
                for (int h = 0; 2 * h < n; ++h) {
                    const double2 v = *reinterpret_cast<const double2 *>(pr + 2 * h);
                    m |= (unsigned)(v.x > min_p) << (2 * h);
                    m |= (unsigned)((2 * h + 1 < n) & (v.y > min_p)) << (2 * h + 1);
                }
            }
        }
        if (ext < V) mask[ext] = (unsigned short)m;
        for (int l = 0; l < n; ++l) {
            const uint64_t b = __ballot((m >> l) & 1u);
            if (lane_id() == 0) s_cnt[wave_id()][l] = __popcll(b);
        }
        __syncthreads();
        if ((int)threadIdx.x < n) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < EX_WAVES; ++w) c += s_cnt[w][threadIdx.x];
            cnt[(size_t)tile * n + threadIdx.x] = c;
        }
        __syncthreads(); // (the counts are read before the next tile overwrites them)
    }
}

// One workgroup of EX_LANES waves. head->offsets[0 .. 16], head->go; base: [tiles][n].
__global__ __launch_bounds__(EX_LANES * WAVE) void k_ex_scan(const int *__restrict__ cnt, int n, int tiles, long long cap,
                                                             long long *__restrict__ base, ExHead *__restrict__ head) {
    __shared__ long long s_total[EX_LANES], s_off[EX_LANES + 1];
    const int l = wave_id(), li = lane_id();
    if (l < n) {
        long long sum = 0;
        for (int t = li; t < tiles; t += WAVE) sum += cnt[(size_t)t * n + l];
        for (int d = WAVE / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (li == 0) s_total[l] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long o = 0;
        for (int i = 0; i <= EX_LANES; ++i) {
            s_off[i] = o;
            head->offsets[i] = o;
            if (i < n) o += s_total[i];
        }
        head->go = o <= cap ? 1 : 0;
        head->pad = 0;
    }
    __syncthreads();
    if (l < n) {
        long long carry = s_off[l];
        for (int t0 = 0; t0 < tiles; t0 += WAVE) { // (a tile holds at most EX_TILE ids: 64 of them sum far inside an int)
            const int t = t0 + li;
            const int c = t < tiles ? cnt[(size_t)t * n + l] : 0;
            const int inc = wave_inclusive_scan(c);
            if (t < tiles) base[(size_t)t * n + l] = carry + (inc - c);
            carry += __builtin_amdgcn_readlane(inc, WAVE - 1);
        }
    }
}

// out_ids / out_p / out_r: head->offsets[n] entries, written only if head->go (out_r may be NULL, then r is too)
__global__ __launch_bounds__(EX_TILE) void k_ex_fill(const double *__restrict__ p, const double *__restrict__ r, int gw, int n,
                                                     const int *__restrict__ ext2int, int V,
                                                     const unsigned short *__restrict__ mask, const long long *__restrict__ base,
                                                     const ExHead *__restrict__ head, int *__restrict__ out_ids,
                                                     double *__restrict__ out_p, double *__restrict__ out_r) {
    __shared__ int s_cnt[EX_WAVES][EX_LANES];
    __shared__ long long s_base[EX_LANES];
    if (!head->go) return;
    const int tiles = (V + EX_TILE - 1) / EX_TILE;
    const int w = wave_id();
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ext = tile * EX_TILE + (int)threadIdx.x;
        const unsigned m = ext < V ? mask[ext] : 0u;
        if (!__syncthreads_or((int)m)) continue; // (the same in every thread of the workgroup)
        for (int l = 0; l < n; ++l) {
            const uint64_t b = __ballot((m >> l) & 1u);
            if (lane_id() == 0) s_cnt[w][l] = __popcll(b);
        }
        if ((int)threadIdx.x < n) s_base[threadIdx.x] = base[(size_t)tile * n + threadIdx.x];
        __syncthreads();
        const int row = m ? ext2int[ext] : 0;
        for (int h = 0; 2 * h < n; ++h) {
            const int l0 = 2 * h, l1 = 2 * h + 1;
            const bool q0 = (m >> l0) & 1u, q1 = l1 < n && ((m >> l1) & 1u);
            const uint64_t b0 = __ballot(q0), b1 = __ballot(q1);
            if ((b0 | b1) == 0) continue; // (wave-uniform)
            if (q0 | q1) {
                const size_t at = (size_t)row * gw + l0;
                double2 vp, vr = make_double2(0.0, 0.0);
                if (gw & 1) { // a single-source slot: rows of one double
                    vp = make_double2(p[at], l1 < gw ? p[at + 1] : 0.0);
                    if (out_r) vr = make_double2(r[at], l1 < gw ? r[at + 1] : 0.0);
                } else {
                    vp = *reinterpret_cast<const double2 *>(p + at);
                    if (out_r) vr = *reinterpret_cast<const double2 *>(r + at);
                }
                if (q0) {
                    long long pos = s_base[l0] + mbcnt(b0);
                    for (int k = 0; k < w; ++k) pos += s_cnt[k][l0];
                    out_ids[pos] = ext;
                    out_p[pos] = vp.x;
                    if (out_r) out_r[pos] = vr.x;
                }
                if (q1) {
                    long long pos = s_base[l1] + mbcnt(b1);
                    for (int k = 0; k < w; ++k) pos += s_cnt[k][l1];
                    out_ids[pos] = ext;
                    out_p[pos] = vp.y;
                    if (out_r) out_r[pos] = vr.y;
                }
            }
        }
        __syncthreads(); // (the counts and bases are read before the next tile overwrites them)
    }
}

template <class T> __device__ __forceinline__ T ex_cvt(double v);
template <> __device__ __forceinline__ double ex_cvt<double>(double v) { return v; }
template <> __device__ __forceinline__ float ex_cvt<float>(double v) { return __double2float_rn(v); }

// src: p or r of the state (rows of gw doubles, n lanes in use). dst: [V][n] or, SOURCE_MAJOR, [n][V]; 0.0 for a vertex without an id.
template <class T, bool SOURCE_MAJOR>
__global__ __launch_bounds__(EX_TILE) void k_ex_dense(const double *__restrict__ src, int gw, int n, const int *__restrict__ ext2int,
                                                      int V, T *__restrict__ dst) {
    if constexpr (!SOURCE_MAJOR) {
        const int64_t total = (int64_t)V * n;
        for (int64_t t = (int64_t)blockIdx.x * EX_TILE + threadIdx.x; t < total; t += (int64_t)gridDim.x * EX_TILE) {
            const int ext = (int)(t / n), lane = (int)(t % n);
            const int row = ext2int[ext];
            dst[t] = ex_cvt<T>(row >= 0 ? src[(size_t)row * gw + lane] : 0.0);
        }
    } else {
        __shared__ double s_v[EX_TILE * (EX_LANES + 1)];
        __shared__ int s_row[EX_TILE];
        const int ls = gw + 1, half = gw / 2;
        const int tiles = (V + EX_TILE - 1) / EX_TILE;
        for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const int e0 = tile * EX_TILE, cnt = min(EX_TILE, V - e0);
            __syncthreads(); // (the stores of the previous tile are over)
            if ((int)threadIdx.x < cnt) s_row[threadIdx.x] = ext2int[e0 + threadIdx.x];
            __syncthreads();
            if (gw & 1) {
                for (int j = threadIdx.x; j < cnt * gw; j += EX_TILE) {
                    const int il = j / gw, l = j % gw, row = s_row[il];
                    s_v[il * ls + l] = row >= 0 ? src[(size_t)row * gw + l] : 0.0;
                }
            } else {
                for (int j = threadIdx.x; j < cnt * half; j += EX_TILE) {
                    const int il = j / half, h = j % half, row = s_row[il];
                    double2 v = make_double2(0.0, 0.0);
                    if (row >= 0) v = *reinterpret_cast<const double2 *>(src + (size_t)row * gw + 2 * h);
                    s_v[il * ls + 2 * h] = v.x;
                    s_v[il * ls + 2 * h + 1] = v.y;
                }
            }
            __syncthreads();
            for (int o = threadIdx.x; o < n * EX_TILE; o += EX_TILE) {
                const int lane = o / EX_TILE, il = o % EX_TILE;
                if (il < cnt) dst[(size_t)lane * V + e0 + il] = ex_cvt<T>(s_v[il * ls + lane]);
            }
        }
    }
}

} // namespace dppr
