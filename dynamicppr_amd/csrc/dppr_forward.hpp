// dppr_forward.hpp -- the forward sweep of dppr_forward: f^K = 0.15 * sum_k x_k for up to 16 starts at once, x_{k+1} a PULL over
// the in-CSR of a resident epoch (Epoch::adj: rows ascend by internal tail id, duplicates kept). Never called from the update
// path; no state of the solver is read. include/dppr.h states every rounding; dppr_forward_plan.hpp restates the row sum on the host.
//
// PLANES, each [V][gw] doubles by internal id, the m columns interleaved as a group's lanes (gw = row_width(m)):
//     y   the per-vertex term of the iteration being read: (0.85 * x_k[u]) / (double)(d(u) + 1)
//     y'  ... of the next one (the two swap per sweep)       f  the accumulated result       x  x_k of a CHECK iteration
// SWEEP k_fw_sweep<PP, LEVELS>, one launch per iteration, no atomic: a SEGMENT of 8 T lanes takes one in-row at a time (8 / T rows
//   share a wave), T the lanes of a team. A team reads one tail's y row -- lane pi its 16-byte pieces pi and pi + T (PP of them) --
//   so a team's access is one coalesced 16 .. 128 bytes and serves every column. The 8 teams of a segment take 8 consecutive
//   entries a round (the next round's entry and row are loaded before this round's is summed), meet by a butterfly (xor T, 2T, 4T:
//   both partners form the same sum) and push the round's sum into a binary counter of partial sums (FwCounter): the tree of the
//   contract, whatever T is. The lanes of team 0 then store: x (check iterations), f = f + 0.15 * x, y' = (0.85 * x) / (d + 1) with
//   the ROW's own out-degree, each column on its own and only where the freeze word -- read once per wave -- lets it.
//   An in-row longer than `piece` entries is LONG and skipped here:
// k_fw_list (once per call) queues the pieces of the long rows (one integer atomic reserves a row's run of the list; where a run
//   lies does not enter any value); k_fw_pieces<PP, LEVELS> gives a segment one queued piece and stores ONE [gw] partial per piece;
//   k_fw_long, a thread per (long row, column), adds a row's partials through the same counter per block of 2^16 entries, the
//   blocks in ascending order, and stores as the sweep does.
// CHECK  k_fw_rem folds the x plane by EXTERNAL id in the tiles of the dot family (h = 1.0: 1.0 * x is x) into partials of
//   k_dot_combine; k_fw_check freezes the columns whose rem <= tol (and, after the last iteration, every column).
// DESIGN.md section 9r has the resource usage and the measurement.
#pragma once

#include "dppr_common.hpp"
#include "dppr_dot.hpp"
#include "dppr_forward_plan.hpp"
#include "dppr_multi.hpp"

namespace dppr {

static_assert(FW_BLOCK == DOT_TILE && FW_BLOCK == 4 * WAVE && Q_LANES == GS_MAX, "a workgroup stages one subtile of the dot family");
static_assert(fw_row_width(1) == row_width(1) && fw_row_width(3) == row_width(3) && fw_row_width(5) == row_width(5) &&
                  fw_row_width(10) == row_width(10) && fw_row_width(16) == row_width(16),
              "dppr_forward_plan.hpp restates row_width");

struct FwGraph { // the epoch's in-CSR and out-degrees by internal id, the live zone
    const int *row_ptr;
    const Adj *adj;
    const int *out_row_ptr;
    int n_int, V;
};

struct FwPlanes {
    const double *y; // read
    double *yn, *f, *x;
    int gw, m;
    int store_x; // a check iteration
};

template <int PP> struct FwVal {
    double2 v[PP];
};
template <int PP> __device__ __forceinline__ FwVal<PP> fw_zero() {
    FwVal<PP> z;
#pragma unroll
    for (int p = 0; p < PP; ++p) z.v[p] = make_double2(0.0, 0.0);
    return z;
}
// left + right, the left operand the earlier entries
template <int PP> __device__ __forceinline__ FwVal<PP> fw_sum(const FwVal<PP> &a, const FwVal<PP> &b) {
    FwVal<PP> s;
#pragma unroll
    for (int p = 0; p < PP; ++p) {
        s.v[p].x = __dadd_rn(a.v[p].x, b.v[p].x);
        s.v[p].y = __dadd_rn(a.v[p].y, b.v[p].y);
    }
    return s;
}

// the binary counter of partial sums: item j meets the 2^k items before it at level k (static indices: registers)
template <int PP, int LEVELS> struct FwCounter {
    FwVal<PP> lvl[LEVELS];
    __device__ __forceinline__ void push(int j, FwVal<PP> v) {
        bool carry = true;
#pragma unroll
        for (int k = 0; k < LEVELS; ++k) {
            const bool bit = (j >> k) & 1;
            if (carry && bit) {
                v = fw_sum<PP>(lvl[k], v);
            } else if (carry) {
                lvl[k] = v;
                carry = false;
            }
        }
    }
    // after n pushes: the occupied levels from the lowest up (the missing ones are padding, +0.0)
    __device__ __forceinline__ FwVal<PP> close(int n) const {
        FwVal<PP> acc = fw_zero<PP>();
        bool have = false;
#pragma unroll
        for (int k = 0; k < LEVELS; ++k)
            if ((n >> k) & 1) {
                acc = have ? fw_sum<PP>(lvl[k], acc) : lvl[k];
                have = true;
            }
        return acc;
    }
};

// where a lane stands in its segment
struct FwLane {
    int T, seg, slot, pi; // lanes of a team; segment of the wave; team of the segment (the entry slot); piece of the team
};
__device__ __forceinline__ FwLane fw_lane(int T) {
    FwLane l;
    l.T = T;
    const int L = FW_SLOTS * T, sl = lane_id() % L;
    l.seg = lane_id() / L;
    l.slot = sl / T;
    l.pi = sl % T;
    return l;
}

// The sum over entries [lo, hi) of adj (hi - lo <= FW_SLOTS << (LEVELS - 1)), in every lane of the segment: this lane's pieces
// pi and pi + T of the [gw] sum.
template <int PP, int LEVELS>
__device__ __forceinline__ FwVal<PP> fw_walk(const FwGraph &g, const double *__restrict__ y, int gw, const FwLane &l, int lo, int hi) {
    const int h = gw / 2;
    auto load = [&](int e) {
        FwVal<PP> v = fw_zero<PP>();
        if (e < hi) {
            const Adj a = g.adj[e];
            if ((unsigned)a.v < (unsigned)g.V) { // (the tail of a stored edge is a row of the planes: always)
                const double2 *row = reinterpret_cast<const double2 *>(y + (size_t)a.v * gw);
#pragma unroll
                for (int p = 0; p < PP; ++p)
                    if (l.pi + p * l.T < h) v.v[p] = row[l.pi + p * l.T];
            }
        }
        return v;
    };
    FwCounter<PP, LEVELS> c;
    FwVal<PP> cur = load(lo + l.slot);
    int j = 0;
    for (int e0 = lo; e0 < hi; e0 += FW_SLOTS, ++j) { // (the same trips in every lane of the segment)
        const FwVal<PP> nxt = load(e0 + FW_SLOTS + l.slot);
        for (int off = l.T; off < FW_SLOTS * l.T; off <<= 1) {
#pragma unroll
            for (int p = 0; p < PP; ++p) {
                cur.v[p].x = __dadd_rn(cur.v[p].x, __shfl_xor(cur.v[p].x, off, WAVE));
                cur.v[p].y = __dadd_rn(cur.v[p].y, __shfl_xor(cur.v[p].y, off, WAVE));
            }
        }
        c.push(j, cur);
        cur = nxt;
    }
    return c.close(j);
}

// one column of a row: x is its sum. frozen: the freeze word.
__device__ __forceinline__ void fw_store_col(const FwPlanes &pl, size_t at, double x, double den) {
    pl.f[at] = __dadd_rn(pl.f[at], __dmul_rn(FW_ALPHA, x));
    pl.yn[at] = __ddiv_rn(__dmul_rn(FW_DAMP, x), den);
    if (pl.store_x) pl.x[at] = x;
}
// the pieces of a row's sum a lane of team 0 holds
template <int PP>
__device__ __forceinline__ void fw_store(const FwPlanes &pl, const FwLane &l, int u, const FwVal<PP> &s, double den, unsigned frozen) {
#pragma unroll
    for (int p = 0; p < PP; ++p) {
        const int c0 = 2 * (l.pi + p * l.T);
        const size_t at = (size_t)u * pl.gw + c0;
        if (c0 < pl.m && !((frozen >> c0) & 1u)) fw_store_col(pl, at, s.v[p].x, den);
        if (c0 + 1 < pl.m && !((frozen >> (c0 + 1)) & 1u)) fw_store_col(pl, at + 1, s.v[p].y, den);
    }
}

// ---- the start of a call ---------------------------------------------------------------------------------------------------------
// one workgroup; the planes and the head are zero, head->starts holds the external ids
__global__ __launch_bounds__(WAVE) void k_fw_init(FwHead *__restrict__ head, int m, int iters, const int *__restrict__ ext2int, FwGraph g,
                                                  double *__restrict__ y, double *__restrict__ f, int gw) {
    if (threadIdx.x != 0) return;
    unsigned frozen = 0;
    for (int c = 0; c < m; ++c) {
        const int q = head->starts[c];
        const int row = (unsigned)q < (unsigned)g.V ? ext2int[q] : -1;
        if (row < 0 || row >= g.V) { // no row: f = 0.15 e_q is the host's to report
            head->rowless[c] = 1;
            head->iters_used[c] = fw_rowless_iters(iters);
            head->rem[c] = 0.0;
            frozen |= 1u << c;
            continue;
        }
        f[(size_t)row * gw + c] = FW_ALPHA;
        if (row < g.n_int) // (a parked row has no edge: its term is never gathered)
            y[(size_t)row * gw + c] = __ddiv_rn(__dmul_rn(FW_DAMP, 1.0), (double)(g.out_row_ptr[row + 1] - g.out_row_ptr[row] + 1));
    }
    head->frozen = frozen;
}

// the long rows and their pieces; grid-stride over the live rows
__global__ __launch_bounds__(FW_BLOCK) void k_fw_list(FwGraph g, int piece, FwHead *__restrict__ head, unsigned long long *__restrict__ items,
                                                      unsigned item_cap, FwLong *__restrict__ longs, unsigned long_cap) {
    for (long long u = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; u < g.n_int; u += (long long)gridDim.x * FW_BLOCK) {
        const int len = g.row_ptr[u + 1] - g.row_ptr[u];
        if (!fw_row_long(len, piece)) continue;
        const unsigned np = (unsigned)fw_pieces(len, piece);
        const unsigned at = atomicAdd(&head->n_long, 1u);
        const unsigned base = atomicAdd(&head->n_items, np);
        if (at >= long_cap || base + np > item_cap) { // (fw_long_cap / fw_item_cap: never)
            head->overflow = 1;
            continue;
        }
        FwLong lr;
        lr.row = (int)u;
        lr.base = base;
        lr.np = np;
        lr.pad = 0;
        longs[at] = lr;
        for (unsigned k = 0; k < np; ++k) items[base + k] = fw_item((unsigned)u, k);
    }
}

// ---- one iteration -----------------------------------------------------------------------------------------------------------------
// grid: fw_units_grid(n_int, T)
template <int PP, int LEVELS>
__global__ __launch_bounds__(FW_BLOCK) void k_fw_sweep(FwGraph g, FwPlanes pl, int T, int piece, const FwHead *__restrict__ head) {
    const unsigned frozen = head->frozen; // (once per wave: the same word in every lane)
    if ((frozen & fw_all(pl.m)) == fw_all(pl.m)) return;
    const FwLane l = fw_lane(T);
    const int wave_rows = WAVE / (FW_SLOTS * T);
    const long long step = (long long)gridDim.x * FW_WAVES * wave_rows;
    for (long long u0 = ((long long)blockIdx.x * FW_WAVES + wave_id()) * wave_rows; u0 < g.n_int; u0 += step) { // (wave-uniform)
        const long long u = u0 + l.seg;
        if (u >= g.n_int) continue; // (no shuffle leaves a segment)
        const int r0 = g.row_ptr[u], r1 = g.row_ptr[u + 1];
        if (fw_row_long(r1 - r0, piece)) continue;
        const FwVal<PP> s = fw_walk<PP, LEVELS>(g, pl.y, pl.gw, l, r0, r1);
        if (l.slot == 0) fw_store<PP>(pl, l, (int)u, s, (double)(g.out_row_ptr[u + 1] - g.out_row_ptr[u] + 1), frozen);
    }
}

// grid-stride, one segment per queued piece. pp [items][gw].
template <int PP, int LEVELS>
__global__ __launch_bounds__(FW_BLOCK) void k_fw_pieces(FwGraph g, const double *__restrict__ y, int gw, int m, int T, int piece,
                                                        const FwHead *__restrict__ head, const unsigned long long *__restrict__ items,
                                                        unsigned item_cap, double *__restrict__ pp) {
    const unsigned frozen = head->frozen;
    if ((frozen & fw_all(m)) == fw_all(m) || head->overflow) return;
    const unsigned n_items = min(head->n_items, item_cap);
    const FwLane l = fw_lane(T);
    const int wave_rows = WAVE / (FW_SLOTS * T), h = gw / 2;
    const long long step = (long long)gridDim.x * FW_WAVES * wave_rows;
    for (long long t0 = ((long long)blockIdx.x * FW_WAVES + wave_id()) * wave_rows; t0 < n_items; t0 += step) {
        const long long t = t0 + l.seg;
        if (t >= n_items) continue;
        const unsigned long long it = items[t];
        const int u = (int)fw_item_row(it);
        const long long k = fw_item_piece(it);
        const int r0 = g.row_ptr[u], r1 = g.row_ptr[u + 1];
        const int lo = r0 + (int)fw_piece_lo(piece, k), hi = r0 + (int)fw_piece_hi(r1 - r0, piece, k);
        const FwVal<PP> s = fw_walk<PP, LEVELS>(g, y, gw, l, lo, hi);
        if (l.slot == 0) {
#pragma unroll
            for (int p = 0; p < PP; ++p)
                if (l.pi + p * l.T < h) *reinterpret_cast<double2 *>(pp + (size_t)t * gw + 2 * (l.pi + p * l.T)) = s.v[p];
        }
    }
}

// grid-stride, one thread per (long row, column)
__global__ __launch_bounds__(FW_BLOCK) void k_fw_long(FwGraph g, FwPlanes pl, int piece, const FwHead *__restrict__ head,
                                                      const FwLong *__restrict__ longs, unsigned long_cap, const double *__restrict__ pp) {
    const unsigned frozen = head->frozen;
    if ((frozen & fw_all(pl.m)) == fw_all(pl.m) || head->overflow) return;
    const long long total = (long long)min(head->n_long, long_cap) * pl.m;
    const int pb = fw_block_pieces(piece);
    for (long long j = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; j < total; j += (long long)gridDim.x * FW_BLOCK) {
        const FwLong lr = longs[j / pl.m];
        const int c = (int)(j % pl.m);
        if ((frozen >> c) & 1u) continue;
        const double *src = pp + (size_t)lr.base * pl.gw + c;
        double acc = 0.0;
        for (unsigned b0 = 0; b0 < lr.np; b0 += (unsigned)pb) {
            FwCounter<1, FW_BLOCK_LEVELS> cnt;
            const int nb = (int)min((unsigned)pb, lr.np - b0);
            for (int k = 0; k < nb; ++k) {
                FwVal<1> v;
                v.v[0] = make_double2(src[(size_t)(b0 + k) * pl.gw], 0.0);
                cnt.push(k, v);
            }
            const double B = cnt.close(nb).v[0].x;
            acc = b0 == 0 ? B : __dadd_rn(acc, B);
        }
        const int u = lr.row;
        fw_store_col(pl, (size_t)u * pl.gw + c, acc, (double)(g.out_row_ptr[u + 1] - g.out_row_ptr[u] + 1));
    }
}

// ---- a check -------------------------------------------------------------------------------------------------------------------------
// The x plane folded by external id: part[c * stride + tile]. dynamic LDS: dot_lds_bytes(gw, 1).
__global__ __launch_bounds__(FW_BLOCK) void k_fw_rem(const double *__restrict__ x, int gw, int m, const int *__restrict__ ext2int, int V,
                                                     double *__restrict__ part, long long stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fw_lds[];
    const int ls = gw + 1, tid = (int)threadIdx.x;
    double *s_x = reinterpret_cast<double *>(fw_lds);
    double *s_h = s_x + DOT_TILE * ls;
    double *s_part = s_h + DOT_HS;
    int *s_row = reinterpret_cast<int *>(s_part + DOT_TILE);
    const int G = dot_groups_dev(m);
    s_h[tid] = 1.0;
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
                int row = tid < cnt ? ext2int[e0 + tid] : -1;
                if (row >= V) row = -1;
                s_row[tid] = row;
                __syncthreads();
                dot_gather_rows(x, gw, s_row, s_x);
                __syncthreads();
                v = dot_subtile(s_h, s_x, s_part, ls, m, m, G);
            }
            sum = carry.push(sub, v);
        }
        if (tid < m) part[(size_t)tid * (size_t)stride + (size_t)tile] = sum;
    }
}

// after iteration k: a column still running whose rem <= tol stops here; `last`: every column does
__global__ __launch_bounds__(WAVE) void k_fw_check(FwHead *__restrict__ head, int m, int k, double tol, int last) {
    if (threadIdx.x != 0) return;
    unsigned frozen = head->frozen;
    for (int c = 0; c < m; ++c) {
        if ((frozen >> c) & 1u) continue;
        const double r = head->cur[c];
        if (last || r <= tol) {
            head->rem[c] = r;
            head->iters_used[c] = k;
            frozen |= 1u << c;
        }
    }
    head->frozen = frozen;
}

// f = 0.15 at the start of a column without a row, in the dense copy
template <class T> __global__ void k_fw_poke(T *__restrict__ dst, long long at) {
    if (threadIdx.x == 0 && blockIdx.x == 0) dst[at] = (T)FW_ALPHA;
}

} // namespace dppr
