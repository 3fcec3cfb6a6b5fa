// dppr_fcluster.hpp -- the full-length conductance sweep (dppr_ftrack_cluster): every qualifying vertex of the window ordered by
// p or by p / (outdeg + 1) and the order swept for its best prefix, with a length bounded by V, not by DPPR_CLUSTER_MAX. Never
// called from the update path. The kernels work on a generic plane (p, gw, m) by internal row -- today the forward planes a track
// was loaded into (k_ft_load); the reverse states can be given the same sweep later. include/dppr.h states every output;
// dppr_fcluster_plan.hpp has the steps of a call and a host restatement.
//
//   k_fc_count  the EXTERNAL ids in tiles of FC_TILE, one id per thread, so id order is the order of the threads: a 16-bit mask per
//               id (bit c: the vertex is live, an edge names it and its score in column c is > min_score) and the tile's counts
//               (a ballot and a popcount per column and wave, the waves combined in LDS). The tiles' counts are scanned by
//               k_ex_scan of dppr_export.hpp, as the sparse export places its entries: no position comes from an atomic.
//   k_fc_fill   (score bits, external id) of every qualifying vertex to base[tile][column] + (the waves before) + mbcnt.
//   (sort)      rocprim::radix_sort_pairs_desc over the 64 bits, one call per column: stable, so equal scores keep ascending id.
//   k_fc_rank   position j of the order's head L into the rank table, one int32 per (live row, column), cleared to -1 by a memset
//               per call; ids and scores to the outputs.
//   k_fc_rows   one wave per position: both rows read coalesced 64 entries at a time, one gather of a rank per entry, the counts
//               wave-uniform (popcount of a ballot) and kept in registers: the differences of dppr_cluster.hpp,
//                   d_out[j] = #{out w : rho(w) > j} - #{in w : rho(w) < j},  d_in[j] = #{in w : rho(w) > j} - #{out w : rho(w) < j},
//               stored once. A row longer than the piece is not walked here: the wave queues its pieces (one integer add reserves
//               the range; where a piece stands in the list enters no value).
//   k_fc_big    one wave per queued piece; its counts join the 64-bit differences by integer atomics (sums: order-free).
//   k_fc_sums / k_fc_carry / k_fc_apply / k_fc_best   the multi-tile prefix sum: a workgroup per tile sums its three arrays, a
//               workgroup per column scans the tiles' sums, a workgroup per tile scans its positions from its carry, writes the
//               prefix arrays, computes phi (one division) and the tile's first minimum, a workgroup per column takes the first
//               minimum over its tiles under (phi ascending, position ascending). No column is scanned by one workgroup alone.
// Every result is written with ordinary vector stores.
#pragma once

#include "dppr_cluster.hpp"
#include "dppr_common.hpp"
#include "dppr_fcluster_plan.hpp"

namespace dppr {

constexpr int FC_TILE_WAVES = FC_TILE / WAVE;
constexpr int FC_ABSENT = 0x7fffffff; // rank of a vertex outside the order: above every position

struct FcGraph { // the epoch's two CSRs by internal id; the live rows are [0, n_int)
    const int *out_row_ptr, *out_col;
    const int *in_row_ptr;
    const Adj *in_adj;
    int n_int;
};

struct FcCtl {        // zeroed per call
    unsigned n_items; // pieces queued by k_fc_rows
    unsigned pad[3];
};

__device__ __forceinline__ double fc_dev_score(int order, double p, int outdeg) {
    return order == DPPR_FCLUSTER_BY_P_OVER_DEG ? __ddiv_rn(p, (double)(outdeg + 1)) : p;
}

// the columns in which external id `ext` qualifies, and (out) its row
__device__ __forceinline__ unsigned fc_mask_of(const double *__restrict__ p, int gw, int m, const int *__restrict__ ext2int, int V, const FcGraph &g,
                                               int order, double min_score, int ext, int *out_row, int *out_deg) {
    const int row = ext < V ? ext2int[ext] : -1;
    *out_row = row;
    *out_deg = 0;
    if ((unsigned)row >= (unsigned)g.n_int) return 0u;
    const int deg = g.out_row_ptr[row + 1] - g.out_row_ptr[row];
    *out_deg = deg;
    if (deg == 0 && g.in_row_ptr[row + 1] == g.in_row_ptr[row]) return 0u; // (no stored edge names it)
    unsigned msk = 0;
    for (int c = 0; c < m; ++c) msk |= (unsigned)(fc_dev_score(order, p[(size_t)row * gw + c], deg) > min_score) << c;
    return msk;
}

// mask: [V] (every id is written), cnt: [tiles][m]
__global__ __launch_bounds__(FC_TILE) void k_fc_count(const double *__restrict__ p, int gw, int m, const int *__restrict__ ext2int, int V, FcGraph g,
                                                      int order, double min_score, unsigned short *__restrict__ mask, int *__restrict__ cnt) {
    __shared__ int s_cnt[FC_TILE_WAVES][Q_LANES];
    const int tiles = (V + FC_TILE - 1) / FC_TILE;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ext = tile * FC_TILE + (int)threadIdx.x;
        int row, deg;
        const unsigned msk = fc_mask_of(p, gw, m, ext2int, V, g, order, min_score, ext, &row, &deg);
        if (ext < V) mask[ext] = (unsigned short)msk;
        for (int c = 0; c < m; ++c) {
            const uint64_t b = __ballot((msk >> c) & 1u);
            if (lane_id() == 0) s_cnt[wave_id()][c] = __popcll(b);
        }
        __syncthreads();
        if ((int)threadIdx.x < m) {
            int n = 0;
#pragma unroll
            for (int w = 0; w < FC_TILE_WAVES; ++w) n += s_cnt[w][threadIdx.x];
            cnt[(size_t)tile * m + threadIdx.x] = n;
        }
        __syncthreads(); // (the counts are read before the next tile overwrites them)
    }
}

// keys / vals: the qualifying entries of column c at [qoff[c], qoff[c + 1]) in ascending external id (base holds qoff[c] already)
__global__ __launch_bounds__(FC_TILE) void k_fc_fill(const double *__restrict__ p, int gw, int m, const int *__restrict__ ext2int, int V, FcGraph g,
                                                     int order, const unsigned short *__restrict__ mask, const long long *__restrict__ base,
                                                     unsigned long long *__restrict__ keys, int *__restrict__ vals) {
    __shared__ int s_cnt[FC_TILE_WAVES][Q_LANES];
    __shared__ long long s_base[Q_LANES];
    const int tiles = (V + FC_TILE - 1) / FC_TILE;
    const int w = wave_id();
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ext = tile * FC_TILE + (int)threadIdx.x;
        const unsigned msk = ext < V ? mask[ext] : 0u;
        if (!__syncthreads_or((int)msk)) continue; // (the same in every thread of the workgroup)
        for (int c = 0; c < m; ++c) {
            const uint64_t b = __ballot((msk >> c) & 1u);
            if (lane_id() == 0) s_cnt[w][c] = __popcll(b);
        }
        if ((int)threadIdx.x < m) s_base[threadIdx.x] = base[(size_t)tile * m + threadIdx.x];
        __syncthreads();
        int row = 0, deg = 0;
        if (msk) {
            row = ext2int[ext];
            deg = g.out_row_ptr[row + 1] - g.out_row_ptr[row];
        }
        for (int c = 0; c < m; ++c) {
            const bool q = (msk >> c) & 1u;
            const uint64_t b = __ballot(q);
            if (q) {
                long long pos = s_base[c] + mbcnt(b);
                for (int k = 0; k < w; ++k) pos += s_cnt[k][c];
                keys[pos] = (unsigned long long)__double_as_longlong(fc_dev_score(order, p[(size_t)row * gw + c], deg));
                vals[pos] = ext;
            }
        }
        __syncthreads(); // (the counts and bases are read before the next tile overwrites them)
    }
}

// the column of absolute position t (m <= 16: a short walk)
__device__ __forceinline__ int fc_col_of(const long long *off, int m, long long t) {
    int c = 0;
    while (c + 1 < m && t >= off[c + 1]) ++c;
    return c;
}

// keys / vals: the sorted entries. rank [n_int][m]; out_ids / out_score [off[m]]
__global__ __launch_bounds__(FC_BLOCK) void k_fc_rank(FcCols cols, const unsigned long long *__restrict__ keys, const int *__restrict__ vals,
                                                      const int *__restrict__ ext2int, int n_int, int *__restrict__ rank, int *__restrict__ out_ids,
                                                      double *__restrict__ out_score) {
    const long long total = cols.off[cols.m];
    for (long long t = (long long)blockIdx.x * FC_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * FC_BLOCK) {
        const int c = fc_col_of(cols.off, cols.m, t);
        const long long j = t - cols.off[c], src = cols.qoff[c] + j;
        const int id = vals[src];
        const int row = ext2int[id];
        if ((unsigned)row < (unsigned)n_int) rank[(size_t)row * cols.m + c] = (int)j; // (a vertex of the order is live: always)
        out_ids[t] = id;
        out_score[t] = __longlong_as_double((long long)keys[src]);
    }
}

// entries [lo, hi) of a row (DIR 0: out_col, 1: in_adj) against position j of column c: how many neighbours rank above it, below it
template <int DIR>
__device__ __forceinline__ void fc_walk(const FcGraph &g, const int *__restrict__ rank, int m, int c, int j, int lo, int hi, int *gt, int *lt) {
    int a = 0, b = 0;
    for (int e0 = lo; e0 < hi; e0 += WAVE) {
        const int e = e0 + lane_id();
        int rho = j; // (a lane past the end: in neither count)
        if (e < hi) {
            const int w = DIR == 0 ? ld_stream(g.out_col + e) : g.in_adj[e].v;
            rho = (unsigned)w < (unsigned)g.n_int ? rank[(size_t)w * m + c] : -1;
            if (rho < 0) rho = FC_ABSENT;
        }
        a += __popcll(__ballot(rho > j));
        b += __popcll(__ballot(rho < j));
    }
    *gt = a;
    *lt = b;
}

// one wave per position, grid-stride. d: d_out [T] | d_in [T] | deg [T], T = off[m]
__global__ __launch_bounds__(FC_BLOCK) void k_fc_rows(FcCols cols, FcGraph g, const int *__restrict__ ext2int, const int *__restrict__ ids,
                                                      const int *__restrict__ rank, int piece, long long *__restrict__ d, FcCtl *__restrict__ ctl,
                                                      FcItem *__restrict__ list, unsigned list_cap) {
    const long long total = cols.off[cols.m];
    for (long long t = (long long)blockIdx.x * FC_WAVES + wave_id(); t < total; t += (long long)gridDim.x * FC_WAVES) {
        const int c = fc_col_of(cols.off, cols.m, t);
        const int j = (int)(t - cols.off[c]);
        long long d_out = 0, d_in = 0, deg = 0;
        const int u = __builtin_amdgcn_readfirstlane(ext2int[ids[t]]);
        if ((unsigned)u < (unsigned)g.n_int) { // (always)
            const int o0 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u]), o1 = __builtin_amdgcn_readfirstlane(g.out_row_ptr[u + 1]);
            const int i0 = __builtin_amdgcn_readfirstlane(g.in_row_ptr[u]), i1 = __builtin_amdgcn_readfirstlane(g.in_row_ptr[u + 1]);
            deg = o1 - o0;
            int gt = 0, lt = 0;
            const unsigned c_out = o1 - o0 > piece ? (unsigned)fc_pieces(o1 - o0, piece) : 0u;
            const unsigned c_in = i1 - i0 > piece ? (unsigned)fc_pieces(i1 - i0, piece) : 0u;
            if (!c_out) {
                fc_walk<0>(g, rank, cols.m, c, j, o0, o1, &gt, &lt);
                d_out += gt;
                d_in -= lt;
            }
            if (!c_in) {
                fc_walk<1>(g, rank, cols.m, c, j, i0, i1, &gt, &lt);
                d_in += gt;
                d_out -= lt;
            }
            const unsigned queued = c_out + c_in; // the pieces this wave hands to k_fc_big: those of its out-row, then those of its in-row
            if (queued) {
                unsigned base = 0;
                if (lane_id() == 0) base = atomicAdd(&ctl->n_items, queued);
                base = __builtin_amdgcn_readfirstlane(base);
                for (unsigned q = lane_id(); q < queued; q += WAVE)
                    if (base + q < list_cap) // (fc_list_cap bounds what a call can queue)
                        list[base + q] = q < c_out ? FcItem{t, q, 0u} : FcItem{t, q - c_out, 1u};
            }
        }
        if (lane_id() == 0) {
            d[t] = d_out;
            d[total + t] = d_in;
            d[2 * total + t] = deg;
        }
    }
}

// fixed grid, one wave per queued piece
__global__ __launch_bounds__(FC_BLOCK) void k_fc_big(FcCols cols, FcGraph g, const int *__restrict__ ext2int, const int *__restrict__ ids,
                                                     const int *__restrict__ rank, int piece, long long *__restrict__ d, const FcCtl *__restrict__ ctl,
                                                     const FcItem *__restrict__ list, unsigned list_cap) {
    const unsigned n_items = min(ctl->n_items, list_cap);
    const long long total = cols.off[cols.m];
    for (unsigned i = blockIdx.x * FC_WAVES + wave_id(); i < n_items; i += gridDim.x * FC_WAVES) {
        const FcItem it = list[i];
        const long long t = it.pos;
        if (t < 0 || t >= total) continue; // (never)
        const int c = fc_col_of(cols.off, cols.m, t);
        const int j = (int)(t - cols.off[c]), dir = (int)it.dir;
        const int u = __builtin_amdgcn_readfirstlane(ext2int[ids[t]]);
        if ((unsigned)u >= (unsigned)g.n_int) continue; // (never)
        const int *rp = dir ? g.in_row_ptr : g.out_row_ptr;
        const int r0 = __builtin_amdgcn_readfirstlane(rp[u]), r1 = __builtin_amdgcn_readfirstlane(rp[u + 1]);
        const long long lo = (long long)r0 + (long long)it.piece * piece;
        const int hi = (int)min((long long)r1, lo + piece);
        int gt = 0, lt = 0;
        if (lo < hi) {
            if (dir) fc_walk<1>(g, rank, cols.m, c, j, (int)lo, hi, &gt, &lt);
            else fc_walk<0>(g, rank, cols.m, c, j, (int)lo, hi, &gt, &lt);
        }
        if (lane_id() == 0) {
            // out-row: (+gt, -lt) into (d_out, d_in); in-row: (-lt, +gt). Two's complement: the sums are those of signed integers
            const long long add_out = dir ? -(long long)lt : (long long)gt, add_in = dir ? (long long)gt : -(long long)lt;
            if (add_out) atomicAdd(reinterpret_cast<unsigned long long *>(&d[t]), (unsigned long long)add_out);
            if (add_in) atomicAdd(reinterpret_cast<unsigned long long *>(&d[total + t]), (unsigned long long)add_in);
        }
    }
}

// tile `tile` (absolute) of the scan: its column, the first position of the tile inside the column and the column's length
__device__ __forceinline__ void fc_tile_of(const FcCols &cols, long long tile, int S, int *c, long long *j0, long long *L) {
    const int col = fc_col_of(cols.tile0, cols.m, tile);
    *c = col;
    *j0 = (tile - cols.tile0[col]) * S;
    *L = cols.off[col + 1] - cols.off[col];
}

// a workgroup per tile: the sums of its three arrays. tsum: [3][tiles]
__global__ __launch_bounds__(FC_BLOCK) void k_fc_sums(FcCols cols, const long long *__restrict__ d, int S, long long *__restrict__ tsum) {
    __shared__ long long s_w[FC_WAVES];
    const long long tiles = cols.tile0[cols.m], total = cols.off[cols.m];
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int c;
        long long j0, L;
        fc_tile_of(cols, tile, S, &c, &j0, &L);
        for (int a = 0; a < 3; ++a) {
            long long x = 0;
            for (int i = threadIdx.x; i < S && j0 + i < L; i += FC_BLOCK) x += d[a * total + cols.off[c] + j0 + i];
            const long long inc = cl_block_scan(x, s_w);
            if (threadIdx.x == FC_BLOCK - 1) tsum[a * tiles + tile] = inc;
        }
    }
}

// a workgroup per column: the exclusive scan of its tiles' sums. carry: [3][tiles]
__global__ __launch_bounds__(FC_BLOCK) void k_fc_carry(FcCols cols, const long long *__restrict__ tsum, long long *__restrict__ carry) {
    __shared__ long long s_w[FC_WAVES];
    __shared__ long long s_tot;
    const int c = blockIdx.x;
    const long long tiles = cols.tile0[cols.m], t0 = cols.tile0[c], n = cols.tile0[c + 1] - t0;
    for (int a = 0; a < 3; ++a) {
        long long before = 0;
        for (long long b = 0; b < n; b += FC_BLOCK) { // (uniform trip count)
            const long long i = b + threadIdx.x;
            const long long x = i < n ? tsum[a * tiles + t0 + i] : 0ll;
            const long long inc = cl_block_scan(x, s_w) + before;
            if (i < n) carry[a * tiles + t0 + i] = inc - x;
            if (threadIdx.x == FC_BLOCK - 1) s_tot = inc;
            __syncthreads();
            before = s_tot;
        }
    }
}

// the first minimum of the workgroup's candidates (LDS tree; every thread returns the winner)
__device__ __forceinline__ FcBest fc_block_best(FcBest mine, FcBest *s_b) {
    __syncthreads(); // (s_b of the previous reduction has been read)
    s_b[threadIdx.x] = mine;
    __syncthreads();
    for (int step = FC_BLOCK / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) {
            const FcBest a = s_b[threadIdx.x], b = s_b[threadIdx.x + step];
            const bool take_b = b.pos >= 0 && (a.pos < 0 || b.phi < a.phi || (b.phi == a.phi && b.pos < a.pos));
            if (take_b) s_b[threadIdx.x] = b;
        }
        __syncthreads();
    }
    return s_b[0];
}

// a workgroup per tile: the prefix sums from the tile's carry, the prefix arrays, phi and the tile's first minimum. tbest: [tiles]
__global__ __launch_bounds__(FC_BLOCK) void k_fc_apply(FcCols cols, const long long *__restrict__ d, const long long *__restrict__ carry, int S,
                                                       long long Ed, int min_size, long long *__restrict__ out_cut_out,
                                                       long long *__restrict__ out_cut_in, long long *__restrict__ out_vol, FcBest *__restrict__ tbest) {
    __shared__ long long s_w[FC_WAVES];
    __shared__ long long s_tot[3];
    __shared__ FcBest s_b[FC_BLOCK];
    const long long tiles = cols.tile0[cols.m], total = cols.off[cols.m];
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int c;
        long long j0, L;
        fc_tile_of(cols, tile, S, &c, &j0, &L);
        long long before[3] = {carry[tile], carry[tiles + tile], carry[2 * tiles + tile]};
        FcBest mine{__builtin_huge_val(), -1, 0, 0};
        for (int b = 0; b < S; b += FC_BLOCK) { // (uniform trip count)
            const int i = b + (int)threadIdx.x;
            const long long j = j0 + i, at = cols.off[c] + j;
            const bool valid = i < S && j < L;
            long long v[3];
            for (int a = 0; a < 3; ++a) v[a] = cl_block_scan(valid ? d[a * total + at] : 0ll, s_w) + before[a];
            if (threadIdx.x == FC_BLOCK - 1)
                for (int a = 0; a < 3; ++a) s_tot[a] = v[a];
            __syncthreads();
            for (int a = 0; a < 3; ++a) before[a] = s_tot[a];
            if (valid) {
                out_cut_out[at] = v[0];
                out_cut_in[at] = v[1];
                out_vol[at] = v[2];
                const long long den = min(v[2], Ed - v[2]);
                if (j + 1 >= (long long)min_size && den > 0) {
                    const double f = __ddiv_rn((double)v[0], (double)den);
                    if (mine.pos < 0 || f < mine.phi) mine = FcBest{f, j, v[0], v[2]}; // (ascending j: the first of equal values stays)
                }
            }
        }
        const FcBest win = fc_block_best(mine, s_b);
        if (threadIdx.x == 0) tbest[tile] = win;
    }
}

// a workgroup per column: the first minimum over its tiles; best [m]
__global__ __launch_bounds__(FC_BLOCK) void k_fc_best(FcCols cols, const FcBest *__restrict__ tbest, dppr_fcluster_t *__restrict__ best) {
    __shared__ FcBest s_b[FC_BLOCK];
    const int c = blockIdx.x;
    const long long t0 = cols.tile0[c], n = cols.tile0[c + 1] - t0;
    FcBest mine{__builtin_huge_val(), -1, 0, 0};
    for (long long i = threadIdx.x; i < n; i += FC_BLOCK) { // (ascending tiles hold ascending positions)
        const FcBest b = tbest[t0 + i];
        if (b.pos >= 0 && (mine.pos < 0 || b.phi < mine.phi)) mine = b;
    }
    const FcBest win = fc_block_best(mine, s_b);
    if (threadIdx.x == 0) {
        dppr_fcluster_t r;
        r.count = cols.off[c + 1] - cols.off[c];
        r.best_size = win.pos < 0 ? 0 : win.pos + 1;
        r.best_cut = win.pos < 0 ? 0 : win.cut;
        r.best_vol = win.pos < 0 ? 0 : win.vol;
        r.best_phi = win.pos < 0 ? __builtin_huge_val() : win.phi;
        best[c] = r;
    }
}

} // namespace dppr
