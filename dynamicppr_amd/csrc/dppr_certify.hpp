// dppr_certify.hpp -- the certificate of a state (dppr_certify / dppr_group_certify): the residual norms of every lane and the
// largest violation of the loop invariant against an epoch's out-CSR. The state is only read. Never called from the update path.
//
// RESIDUAL PASS  k_cert_residual: one streaming pass by EXTERNAL id, in the tiles of the dot family (dppr_dot_plan.hpp: 2048 ids a
//   tile, 256 a subtile), because the two sums are that family's fold: a subtile's rows come through ext2int, LW threads share a
//   row (LW: the lanes rounded up to a power of two; consecutive threads, consecutive doubles of a row), a thread classifies its
//   (row, lane) -- not finite, r > eps, r < -eps, p != 0, the word of |r| against the largest it has met -- and stages |r|, then p,
//   as the terms of dot_subtile with h = 1.0 (1.0 * x is x: the fold is the dot family's, the transform is applied on the way into
//   LDS). The tile sums leave through DotCarry as partials of k_dot_combine. A row that is not finite stages +0.0 twice.
//   Counts are integer sums: the threads of a lane meet by a butterfly inside a wave, the waves in LDS, a workgroup adds once per
//   lane with a 64-bit integer atomic. Maximum and arg-max: the bit pattern of a non-negative finite double orders like an
//   unsigned 64-bit integer, so (word descending, external id ascending) is a total order without a floating-point compare; it is
//   reduced the same way and every workgroup stores ONE (word, id) per lane with plain stores (CertMax) for k_cert_finish.
// INVARIANT PASS, four launches, none waits for another workgroup:
//   k_cert_rows    the gather S[u] = sum of p[w] over the stored out-edges u -> w, for every live row. A wave takes wave_rows
//                  rows at a time, every row a segment of 64 / wave_rows lanes; a segment is teams of T lanes, lane j of a team
//                  reads 16 bytes (double2 j) of a head's row, so a team reads one head's row in one coalesced 16 .. 128-byte
//                  access that serves every lane of the group, and a segment takes 64 / wave_rows / T heads per step. A team adds
//                  its heads in row order; the teams of a segment meet by a butterfly in a fixed order (xor T, 2T, ..). A row
//                  longer than `piece` edges is LONG: the segment queues its pieces (one 32-bit integer atomic reserves a
//                  contiguous run of the list) and sums nothing.
//   k_cert_pieces  one wave per queued piece, the whole wave one segment; ONE [gw] partial per piece, plain stores.
//   k_cert_long    a thread per (queued piece, column): the thread of a row's piece 0 adds the row's partials in piece order.
//   k_cert_err     by external id as the residual pass: err = |(p + 0.15 r) - (0.15 h + (0.85 S) / (double)(d + 1))|, every
//                  operation rounded where it stands; (word of err, id) reduced as above. An err that is not finite takes no part.
// k_cert_finish: one wave per lane folds the workgroups' (word, id) partials and writes the planes the call asked for.
// No floating-point atomic anywhere; the order of the additions inside S depends on (piece, wave_rows) alone, never on the grid.
// DESIGN.md section 9o has the resource usage and the measurement.
#pragma once

#include "dppr_common.hpp"
#include "dppr_certify_plan.hpp"
#include "dppr_dot.hpp"
#include "dppr_explain.hpp"

namespace dppr {

static_assert(CERT_BLOCK == DOT_TILE && CERT_BLOCK == 4 * WAVE && Q_LANES == GS_MAX, "a workgroup stages one subtile of the dot family");

constexpr int CERT_NO_ID = 0x7fffffff;

struct CertGraph { // the epoch's out-CSR by internal id and the live zone
    const int *out_row_ptr, *out_col;
    int n_int, V;
};

struct CertOut { // the planes of the block, [n] each; NULL: not asked for
    double *max_abs_r, *sum_abs_r, *sum_p, *inv_max_err;
    long long *n_pos, *n_neg, *n_nonfinite, *n_p_nonzero;
    int *argmax_r, *inv_argmax;
};

// (wa, ia) strictly before (wb, ib): the larger word, the smaller id among equals
__device__ __forceinline__ bool cert_before(unsigned long long wa, int ia, unsigned long long wb, int ib) {
    return wa > wb || (wa == wb && ia < ib);
}

// The (word, id) of the threads of a workgroup that share a lane (tid % LW) -> out[lane], by thread tid < LW. Called by all.
__device__ __forceinline__ void cert_wg_max(unsigned long long w, int id, int LW, CertMax *s_max, CertMax *out) {
    for (int off = LW; off < WAVE; off <<= 1) {
        const unsigned long long ow = __shfl_xor(w, off, WAVE);
        const int oid = __shfl_xor(id, off, WAVE);
        if (cert_before(ow, oid, w, id)) {
            w = ow;
            id = oid;
        }
    }
    if (lane_id() < LW) {
        s_max[wave_id() * Q_LANES + lane_id()].word = w;
        s_max[wave_id() * Q_LANES + lane_id()].id = id;
    }
    __syncthreads();
    if ((int)threadIdx.x < LW) {
        for (int k = 1; k < CERT_WAVES; ++k) {
            const CertMax o = s_max[k * Q_LANES + threadIdx.x];
            if (cert_before(o.word, o.id, w, id)) {
                w = o.word;
                id = o.id;
            }
        }
        out[threadIdx.x].word = w;
        out[threadIdx.x].id = id;
        out[threadIdx.x].pad = 0;
    }
}

// ... and a count of theirs -> one integer atomic per lane
__device__ __forceinline__ void cert_wg_count(unsigned long long c, int LW, int n, unsigned long long *s_cnt, unsigned long long *dst) {
    for (int off = LW; off < WAVE; off <<= 1) c += __shfl_xor(c, off, WAVE);
    __syncthreads(); // (s_cnt of the previous count has been read)
    if (lane_id() < LW) s_cnt[wave_id() * Q_LANES + lane_id()] = c;
    __syncthreads();
    if ((int)threadIdx.x < LW && (int)threadIdx.x < n) {
        for (int k = 1; k < CERT_WAVES; ++k) c += s_cnt[k * Q_LANES + threadIdx.x];
        if (c) atomicAdd(dst + threadIdx.x, c);
    }
}

// ---- the residual pass -----------------------------------------------------------------------------------------------------
// grid: cert_stream_grid(V) <= CERT_GRID_MAX. part[(which * n + i) * stride + tile], which 0: |r|, 1: p. wg_max[blockIdx.x][16].
// dynamic LDS: rows [256][n + 1], h [257], partials [256] (doubles), row ids [256] (int)
__global__ __launch_bounds__(CERT_BLOCK) void k_cert_residual(const double *__restrict__ p, const double *__restrict__ r, int gw, int n,
                                                              const int *__restrict__ ext2int, int V, double eps,
                                                              double *__restrict__ part, long long stride, CertHead *__restrict__ head,
                                                              CertMax *__restrict__ wg_max) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cert_lds[];
    __shared__ CertMax s_max[CERT_WAVES * Q_LANES];
    __shared__ unsigned long long s_cnt[CERT_WAVES * Q_LANES];
    const int ls = n + 1, tid = (int)threadIdx.x;
    double *s_x = reinterpret_cast<double *>(cert_lds);
    double *s_h = s_x + DOT_TILE * ls;
    double *s_part = s_h + DOT_HS;
    int *s_row = reinterpret_cast<int *>(s_part + DOT_TILE);
    const int LW = cert_lane_stride(n), RG = CERT_BLOCK / LW, gq = tid / LW, l = tid % LW;
    const int G = dot_groups_dev(n);
    const bool lane_on = l < n;
    s_h[tid] = 1.0;
    unsigned long long c_pos = 0, c_neg = 0, c_nf = 0, c_nz = 0, mw = 0;
    int mid = CERT_NO_ID;
    const long long tiles = ((long long)V + DOT_WG_SLOTS - 1) / DOT_WG_SLOTS;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        DotCarry carry_r, carry_p;
        double sum_r = 0.0, sum_p = 0.0;
        for (int sub = 0; sub < DOT_SUB; ++sub) {
            const long long e0 = tile * DOT_WG_SLOTS + (long long)sub * DOT_TILE;
            const int cnt = (int)min((long long)DOT_TILE, (long long)V - e0);
            double vr = 0.0, vp = 0.0; // (a subtile of padding)
            if (cnt > 0) {
                __syncthreads(); // (the fold of the previous subtile is over)
                s_row[tid] = tid < cnt ? ext2int[e0 + tid] : -1;
                __syncthreads();
                double pk[Q_LANES];
#pragma unroll
                for (int k = 0; k < Q_LANES; ++k) {
                    pk[k] = 0.0;
                    if (k < LW && lane_on) {
                        const int il = gq + k * RG, row = s_row[il];
                        double rv = 0.0, pv = 0.0;
                        if (row >= 0) {
                            rv = r[(size_t)row * gw + l];
                            pv = p[(size_t)row * gw + l];
                            if (__builtin_isfinite(rv) && __builtin_isfinite(pv)) {
                                c_pos += rv > eps ? 1 : 0;
                                c_neg += rv < -eps ? 1 : 0;
                                c_nz += pv != 0.0 ? 1 : 0;
                                const unsigned long long w = (unsigned long long)__double_as_longlong(fabs(rv));
                                const int ext = (int)(e0 + il);
                                if (cert_before(w, ext, mw, mid)) {
                                    mw = w;
                                    mid = ext;
                                }
                            } else {
                                c_nf += 1;
                                rv = 0.0;
                                pv = 0.0;
                            }
                        }
                        s_x[il * ls + l] = fabs(rv);
                        pk[k] = pv;
                    }
                }
                __syncthreads();
                vr = dot_subtile(s_h, s_x, s_part, ls, n, n, G);
                __syncthreads(); // (every term of |r| has been read)
#pragma unroll
                for (int k = 0; k < Q_LANES; ++k)
                    if (k < LW && lane_on) s_x[(gq + k * RG) * ls + l] = pk[k];
                __syncthreads();
                vp = dot_subtile(s_h, s_x, s_part, ls, n, n, G);
            }
            sum_r = carry_r.push(sub, vr);
            sum_p = carry_p.push(sub, vp);
        }
        if (tid < n) {
            part[(size_t)tid * (size_t)stride + (size_t)tile] = sum_r;
            part[(size_t)(n + tid) * (size_t)stride + (size_t)tile] = sum_p;
        }
    }
    __syncthreads();
    cert_wg_count(c_pos, LW, n, s_cnt, head->n_pos);
    cert_wg_count(c_neg, LW, n, s_cnt, head->n_neg);
    cert_wg_count(c_nf, LW, n, s_cnt, head->n_nonfinite);
    cert_wg_count(c_nz, LW, n, s_cnt, head->n_p_nonzero);
    cert_wg_max(mw, mid, LW, s_max, wg_max + (size_t)blockIdx.x * Q_LANES);
}

// ---- the gather of the invariant pass ------------------------------------------------------------------------------------
// The heads of entries [lo, hi) this lane's team takes (entry lo + team, then every `teams`-th), added in row order: double2 `pi`
// of every head's row (a slot: the one double). Four heads in flight per round trip; the order of the additions is the row's.
__device__ __forceinline__ double2 cert_walk(const double *__restrict__ p, int gw, const CertGraph &g, int lo, int hi, int team, int teams,
                                             int pi, bool col_on) {
    double2 acc = make_double2(0.0, 0.0);
    if (!col_on) return acc;
    auto row = [&](int e) {
        const int w = ld_stream(g.out_col + e);
        double2 v = make_double2(0.0, 0.0);
        if ((unsigned)w < (unsigned)g.V) { // (the head of a stored edge is a row of the state: always)
            if (gw == 1)
                v.x = p[w];
            else
                v = *reinterpret_cast<const double2 *>(p + (size_t)w * gw + 2 * pi);
        }
        return v;
    };
    auto add = [&](const double2 &v) {
        acc.x = __dadd_rn(acc.x, v.x);
        acc.y = __dadd_rn(acc.y, v.y);
    };
    int e = lo + team;
    for (; e < hi - 3 * teams; e += 4 * teams) {
        const double2 v0 = row(e), v1 = row(e + teams), v2 = row(e + 2 * teams), v3 = row(e + 3 * teams);
        add(v0);
        add(v1);
        add(v2);
        add(v3);
    }
    for (; e < hi; e += teams) add(row(e));
    return acc;
}
// the teams of a segment of L lanes meet: xor T, 2T, .. L / 2 (both partners form the same sum: + commutes)
__device__ __forceinline__ double2 cert_meet(double2 acc, int T, int L) {
    for (int off = T; off < L; off <<= 1) {
        acc.x = __dadd_rn(acc.x, __shfl_xor(acc.x, off, WAVE));
        acc.y = __dadd_rn(acc.y, __shfl_xor(acc.y, off, WAVE));
    }
    return acc;
}
__device__ __forceinline__ void cert_store(double *dst, int gw, int pi, const double2 &v) {
    if (gw == 1)
        dst[0] = v.x;
    else
        *reinterpret_cast<double2 *>(dst + 2 * pi) = v;
}

// grid: cert_rows_grid(n_int, wave_rows). S [n_int][gw]. items [cap]: the pieces of the long rows (head->n_items of them).
__global__ __launch_bounds__(CERT_BLOCK) void k_cert_rows(const double *__restrict__ p, int gw, CertGraph g, int piece, int wave_rows,
                                                          double *__restrict__ S, CertHead *__restrict__ head,
                                                          unsigned long long *__restrict__ items, unsigned cap) {
    const int T = cert_team(gw), L = WAVE / wave_rows, teams = L / T;
    const int seg = lane_id() / L, sl = lane_id() % L, team = sl / T, pi = sl % T;
    const bool col_on = gw == 1 ? pi == 0 : 2 * pi < gw;
    const long long step = (long long)gridDim.x * CERT_WAVES * wave_rows;
    for (long long u0 = ((long long)blockIdx.x * CERT_WAVES + wave_id()) * wave_rows; u0 < g.n_int; u0 += step) { // (wave-uniform)
        const long long u = u0 + seg;
        int r0 = 0, r1 = 0;
        if (u < g.n_int) {
            r0 = g.out_row_ptr[u];
            r1 = g.out_row_ptr[u + 1];
        }
        if (cert_row_long(r1 - r0, piece)) {
            if (sl == 0) {
                const unsigned np = (unsigned)cert_row_pieces(r1 - r0, piece);
                const unsigned base = atomicAdd(&head->n_items, np);
                if (base + np <= cap) // (cert_list_cap: always)
                    for (unsigned k = 0; k < np; ++k) items[base + k] = cert_item((unsigned)u, k);
            }
            continue; // (no shuffle below needs this segment: cert_meet stays inside a segment)
        }
        const double2 acc = cert_meet(cert_walk(p, gw, g, r0, r1, team, teams, pi, col_on), T, L);
        if (u < g.n_int && team == 0 && col_on) cert_store(S + (size_t)u * gw, gw, pi, acc);
    }
}

// grid-stride, one wave per queued piece. pp [items][gw].
__global__ __launch_bounds__(CERT_BLOCK) void k_cert_pieces(const double *__restrict__ p, int gw, CertGraph g, int piece,
                                                            const CertHead *__restrict__ head, const unsigned long long *__restrict__ items,
                                                            unsigned cap, double *__restrict__ pp) {
    const int T = cert_team(gw), teams = WAVE / T, team = lane_id() / T, pi = lane_id() % T;
    const bool col_on = gw == 1 ? pi == 0 : 2 * pi < gw;
    const unsigned n_items = min(head->n_items, cap);
    for (unsigned t = blockIdx.x * CERT_WAVES + wave_id(); t < n_items; t += gridDim.x * CERT_WAVES) {
        const unsigned long long it = items[t];
        const int u = (int)cert_item_row(it);
        const long long k = cert_item_piece(it);
        const int r0 = g.out_row_ptr[u], r1 = g.out_row_ptr[u + 1];
        const int lo = r0 + (int)cert_piece_lo(piece, k), hi = r0 + (int)cert_piece_hi(r1 - r0, piece, k);
        const double2 acc = cert_meet(cert_walk(p, gw, g, lo, hi, team, teams, pi, col_on), T, WAVE);
        if (team == 0 && col_on) cert_store(pp + (size_t)t * gw, gw, pi, acc);
    }
}

// grid-stride, one thread per (queued piece, column): a row's partials lie side by side, in piece order
__global__ __launch_bounds__(CERT_BLOCK) void k_cert_long(int gw, CertGraph g, int piece, const CertHead *__restrict__ head,
                                                          const unsigned long long *__restrict__ items, unsigned cap,
                                                          const double *__restrict__ pp, double *__restrict__ S) {
    const long long total = (long long)min(head->n_items, cap) * gw;
    for (long long j = (long long)blockIdx.x * CERT_BLOCK + threadIdx.x; j < total; j += (long long)gridDim.x * CERT_BLOCK) {
        const long long t = j / gw;
        const int c = (int)(j % gw);
        const unsigned long long it = items[t];
        if (cert_item_piece(it) != 0) continue;
        const int u = (int)cert_item_row(it);
        const long long np = cert_row_pieces(g.out_row_ptr[u + 1] - g.out_row_ptr[u], piece);
        double sum = pp[(size_t)t * gw + c];
        for (long long k = 1; k < np; ++k) sum = __dadd_rn(sum, pp[(size_t)(t + k) * gw + c]);
        S[(size_t)u * gw + c] = sum;
    }
}

// ---- the violation of the invariant ----------------------------------------------------------------------------------------
// grid <= CERT_GRID_MAX. wg_max[blockIdx.x][16].
__global__ __launch_bounds__(CERT_BLOCK) void k_cert_err(const double *__restrict__ p, const double *__restrict__ r, int gw, int n,
                                                         const int *__restrict__ ext2int, int V, CertGraph g, RkLanes lanes,
                                                         const double *__restrict__ S, CertMax *__restrict__ wg_max) {
    __shared__ CertMax s_max[CERT_WAVES * Q_LANES];
    const int LW = cert_lane_stride(n), RG = CERT_BLOCK / LW, gq = (int)threadIdx.x / LW, l = (int)threadIdx.x % LW;
    unsigned long long mw = 0;
    int mid = CERT_NO_ID;
    if (l < n)
        for (long long v = (long long)blockIdx.x * RG + gq; v < V; v += (long long)gridDim.x * RG) {
            const int u = ext2int[v];
            if (u < 0) continue; // (no id: p = r = h = 0)
            double s = 0.0, den = 1.0; // (a parked row: d = 0, S = 0)
            if (u < g.n_int) {
                s = S[(size_t)u * gw + l];
                den = (double)(g.out_row_ptr[u + 1] - g.out_row_ptr[u] + 1);
            }
            const double lhs = __dadd_rn(p[(size_t)u * gw + l], __dmul_rn(ALPHA, r[(size_t)u * gw + l]));
            const double rhs = __dadd_rn(__dmul_rn(ALPHA, ex_h(lanes, l, u)), __ddiv_rn(__dmul_rn(ONE_MINUS_ALPHA, s), den));
            const double err = fabs(__dsub_rn(lhs, rhs));
            if (!__builtin_isfinite(err)) continue;
            const unsigned long long w = (unsigned long long)__double_as_longlong(err);
            if (cert_before(w, (int)v, mw, mid)) {
                mw = w;
                mid = (int)v;
            }
        }
    cert_wg_max(mw, mid, LW, s_max, wg_max + (size_t)blockIdx.x * Q_LANES);
}

// ---- the planes of the block -----------------------------------------------------------------------------------------------
// grid: n workgroups of one wave, lane i = blockIdx.x. nwg_r / nwg_inv: workgroups of the two streaming passes (0: not run).
__global__ __launch_bounds__(WAVE) void k_cert_finish(const CertHead *__restrict__ head, const double *__restrict__ sums, int n,
                                                      const CertMax *__restrict__ max_r, int nwg_r, const CertMax *__restrict__ max_inv,
                                                      int nwg_inv, CertOut o) {
    const int i = (int)blockIdx.x;
    auto fold = [&](const CertMax *src, int nwg, unsigned long long &w, int &id) {
        w = 0;
        id = CERT_NO_ID;
        for (int k = lane_id(); k < nwg; k += WAVE) {
            const CertMax m = src[(size_t)k * Q_LANES + i];
            if (cert_before(m.word, m.id, w, id)) {
                w = m.word;
                id = m.id;
            }
        }
        for (int off = 1; off < WAVE; off <<= 1) {
            const unsigned long long ow = __shfl_xor(w, off, WAVE);
            const int oid = __shfl_xor(id, off, WAVE);
            if (cert_before(ow, oid, w, id)) {
                w = ow;
                id = oid;
            }
        }
    };
    unsigned long long w;
    int id;
    if (nwg_r > 0) {
        fold(max_r, nwg_r, w, id);
        if (lane_id() == 0) {
            if (o.max_abs_r) o.max_abs_r[i] = __longlong_as_double((long long)w);
            if (o.argmax_r) o.argmax_r[i] = id == CERT_NO_ID ? -1 : id;
            if (o.sum_abs_r) o.sum_abs_r[i] = sums[i];
            if (o.sum_p) o.sum_p[i] = sums[n + i];
            if (o.n_pos) o.n_pos[i] = (long long)head->n_pos[i];
            if (o.n_neg) o.n_neg[i] = (long long)head->n_neg[i];
            if (o.n_nonfinite) o.n_nonfinite[i] = (long long)head->n_nonfinite[i];
            if (o.n_p_nonzero) o.n_p_nonzero[i] = (long long)head->n_p_nonzero[i];
        }
    }
    if (nwg_inv > 0) {
        fold(max_inv, nwg_inv, w, id);
        if (lane_id() == 0) {
            if (o.inv_max_err) o.inv_max_err[i] = __longlong_as_double((long long)w);
            if (o.inv_argmax) o.inv_argmax[i] = id == CERT_NO_ID ? -1 : id;
        }
    }
}

} // namespace dppr
