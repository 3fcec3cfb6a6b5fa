// dppr_fpush.hpp -- the forward push of dppr_forward_push: the frontier-driven push of Andersen, Chung and Lang for up to 16
// weighted start sets at once over a resident epoch. Never called from the update path; no state of the solver is read.
// include/dppr.h states every rounding; dppr_fpush_plan.hpp has the round, the lists and a host restatement.
//
// PLANES, each [V][gw] doubles by internal id, the m columns interleaved as a group's lanes: p | r | y0 | y1 (the planes of
// dppr_forward). Round k writes and reads y[k & 1] and clears the other one, so no row is cleared while it is read.
// LISTS of internal ids, two of each, alternating by k & 1: front (rows with any column pushed in the round), recv (rows with at
// least one in-neighbour in front: the candidates of the next round). A bit per row makes a row enter recv once.
// THE LISTS ARE SETS: where a row stands in a list decides only which lanes handle it. A value of p, r or y is written by the one
// thread (or the one segment) that owns its row in that launch, from values that no other thread of the launch writes; the
// integer counters (pushes, left, work, list lengths) are sums of integers. So the order of a list enters no value, and no
// floating-point atomic exists in this file.
// k_fp_init    the seed table: ext2int, r = w, the rows enter recv[0]; a seed without a row (no internal id, parked, or named by
//              no stored edge of the epoch) is flagged for the host.
// k_fp_select  a thread per candidate: r > thr per column, p, y, r; a ballot and ONE integer atomic per wave append the pushed
//              rows to front and the pieces of their out-rows to the mark list; clears the bits of the candidates and the other
//              y plane of the previous frontier.
// k_fp_mark    16 lanes per piece of <= 128 out-edges (a hub in pieces): atomicOr sets the head's bit, the first setter enters
//              recv -- a long in-row also the piece lists of dppr_forward.hpp -- and counts the row's in-edges.
// k_fp_gather  a segment per receiver: fw_walk / FwCounter over y, r += sum per column; long rows go through k_fw_pieces and
//              k_fp_long (the counter over the pieces' partials, the blocks ascending: k_fw_long with another store).
// k_fp_left    after the last round: the candidates still above thr, per column.
// Every round kernel takes its counts from device memory and loops grid-stride: a round after convergence is empty launches.
// DESIGN.md section 9s has the resource usage and the measurement.
#pragma once

#include "dppr_forward.hpp"
#include "dppr_fpush_plan.hpp"

namespace dppr {

struct FpLists {
    int *front[2], *recv[2];
    unsigned *bits;
    unsigned long long *mark; // fw_item(row, piece of its out-row)
    unsigned list_cap, mark_cap;
};

// exclusive prefix sum of v over the wave; total in every lane
__device__ __forceinline__ unsigned fp_wave_scan(unsigned v, unsigned &total) {
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const unsigned o = __shfl_up(inc, off, WAVE);
        if (lane_id() >= off) inc += o;
    }
    total = __shfl(inc, WAVE - 1, WAVE);
    return inc - v;
}

// grid-stride over the seeds; the planes, the bitmap and the head are zero
__global__ __launch_bounds__(FW_BLOCK) void k_fp_init(FpHead *__restrict__ head, FpSeed *__restrict__ seeds, int n_seeds,
                                                      const int *__restrict__ ext2int, FwGraph g, double *__restrict__ r, int gw, FpLists ls) {
    for (long long j = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; j < n_seeds; j += (long long)gridDim.x * FW_BLOCK) {
        const FpSeed s = seeds[j];
        int row = (unsigned)s.id < (unsigned)g.V ? ext2int[s.id] : -1;
        if (row >= g.n_int) row = -1; // parked
        // a live row that no stored edge of the epoch names is no row either: what a column is does not depend on whether a
        // vertex without an edge happens to be parked, so a seed that a later batch revives is answered the same way
        if (row >= 0 && g.row_ptr[row + 1] == g.row_ptr[row] && g.out_row_ptr[row + 1] == g.out_row_ptr[row]) row = -1;
        if (row < 0) { // p = 0.15 w is the host's to report
            seeds[j].row = -1;
            continue;
        }
        seeds[j].row = row;
        r[(size_t)row * gw + s.col] = s.w; // (an id stands once in a column)
        const unsigned bit = 1u << (row & 31);
        if (!(atomicOr(&ls.bits[row >> 5], bit) & bit)) {
            const unsigned at = atomicAdd(&head->n_recv[0], 1u);
            if (at < ls.list_cap) ls.recv[0][at] = row;
            else head->overflow = 1;
        }
    }
}

// round k, b = k & 1: candidates recv[b ^ 1] -> front[b], the mark list; y[b ^ 1] of front[b ^ 1] cleared.
// SIGNED (the forward track, dppr_ftrack.hpp): the test is |r| > thr; the push is the same three assignments.
template <bool SIGNED>
__global__ __launch_bounds__(FW_BLOCK) void k_fp_select(FpHead *__restrict__ head, FwGraph g, double eps, double *__restrict__ p,
                                                        double *__restrict__ r, double *__restrict__ y, double *__restrict__ y_old, int gw, int m,
                                                        FpLists ls, int b) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { // (written by the mark of this round, read by nothing before it)
        head->fw.n_items = 0;
        head->fw.n_long = 0;
    }
    const unsigned n = min(head->n_recv[b ^ 1], ls.list_cap);
    const int *cand = ls.recv[b ^ 1];
    const long long step = (long long)gridDim.x * FW_BLOCK;
    unsigned act = 0;
    for (long long i0 = (long long)blockIdx.x * FW_BLOCK + wave_id() * WAVE; i0 < n; i0 += step) { // (wave-uniform)
        const long long i = i0 + lane_id();
        unsigned mask = 0, np = 0;
        int u = -1;
        if (i < n) {
            u = cand[i];
            if ((unsigned)u >= (unsigned)g.n_int) u = -1; // (a list holds live rows: never)
        }
        if (u >= 0) {
            atomicAnd(&ls.bits[u >> 5], ~(1u << (u & 31)));
            const int deg = g.out_row_ptr[u + 1] - g.out_row_ptr[u];
            const double den = (double)(deg + 1), thr = __dmul_rn(eps, den);
            const size_t at = (size_t)u * gw;
            for (int c = 0; c < m; ++c) {
                const double rv = r[at + c];
                if ((SIGNED ? fabs(rv) : rv) > thr) {
                    p[at + c] = __dadd_rn(p[at + c], __dmul_rn(FW_ALPHA, rv));
                    y[at + c] = __ddiv_rn(__dmul_rn(FW_DAMP, rv), den);
                    r[at + c] = 0.0;
                    mask |= 1u << c;
                }
            }
            if (mask) np = (unsigned)fp_mark_pieces(deg);
        }
        const unsigned long long pushed = __ballot(mask != 0);
        if (pushed) { // (wave-uniform)
            const unsigned cnt = (unsigned)__popcll(pushed), rank = (unsigned)__popcll(pushed & ((1ull << lane_id()) - 1ull));
            unsigned np_all;
            const unsigned np_at = fp_wave_scan(np, np_all);
            unsigned base = 0, mbase = 0;
            if (lane_id() == 0) {
                base = atomicAdd(&head->n_front[b], cnt);
                if (np_all) mbase = atomicAdd(&head->n_mark, np_all);
            }
            base = __shfl(base, 0, WAVE);
            mbase = __shfl(mbase, 0, WAVE);
            if (mask) {
                if (base + rank < ls.list_cap && mbase + np_at + np <= ls.mark_cap) {
                    ls.front[b][base + rank] = u;
                    for (unsigned k = 0; k < np; ++k) ls.mark[mbase + np_at + k] = fw_item((unsigned)u, k);
                } else {
                    head->overflow = 1;
                }
            }
            for (int c = 0; c < m; ++c) {
                const unsigned long long in_c = __ballot((mask >> c) & 1u);
                if (in_c) {
                    act |= 1u << c;
                    if (lane_id() == 0) atomicAdd(&head->pushes[c], (unsigned long long)__popcll(in_c));
                }
            }
        }
    }
    if (act && lane_id() == 0) atomicOr(&head->act, act);
    // the other y plane: the frontier of the round before
    const unsigned n_old = min(head->n_front[b ^ 1], ls.list_cap);
    const long long total = (long long)n_old * gw;
    for (long long t = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; t < total; t += step) {
        const int u = ls.front[b ^ 1][t / gw];
        if ((unsigned)u < (unsigned)g.V) y_old[(size_t)u * gw + t % gw] = 0.0;
    }
}

// round k: the mark list -> the bits, recv[b], the piece lists of the long receivers
__global__ __launch_bounds__(FW_BLOCK) void k_fp_mark(FpHead *__restrict__ head, FwGraph g, const int *__restrict__ out_col, FpLists ls, int b,
                                                      int piece, unsigned long long *__restrict__ items, unsigned item_cap,
                                                      FwLong *__restrict__ longs, unsigned long_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { // (select of this round is over; nothing below reads these)
        const unsigned act = head->act;
        for (int c = 0; c < Q_LANES; ++c)
            if ((act >> c) & 1u) head->rounds_used[c] += 1;
        head->last_act = act;
        head->act = 0;
        head->work[0] += head->n_front[b];
        head->n_recv[b ^ 1] = 0;
        head->n_front[b ^ 1] = 0;
    }
    const unsigned n = min(head->n_mark, ls.mark_cap);
    constexpr int SUBS = WAVE / FP_MARK_LANES;
    const int sub = lane_id() / FP_MARK_LANES, sl = lane_id() % FP_MARK_LANES;
    const long long step = (long long)gridDim.x * FW_WAVES * SUBS;
    unsigned long long edges = 0;
    for (long long t0 = ((long long)blockIdx.x * FW_WAVES + wave_id()) * SUBS; t0 < n; t0 += step) { // (wave-uniform)
        const long long t = t0 + sub;
        int lo = 0, hi = 0;
        if (t < n) {
            const unsigned long long it = ls.mark[t];
            const unsigned u = fw_item_row(it);
            if (u < (unsigned)g.n_int) {
                const int o0 = g.out_row_ptr[u], o1 = g.out_row_ptr[u + 1];
                lo = o0 + (int)fw_item_piece(it) * FP_MARK_PIECE;
                hi = min(lo + FP_MARK_PIECE, o1);
            }
        }
        for (int j = 0; j < FP_MARK_PIECE; j += FP_MARK_LANES) {
            const int e = lo + j + sl;
            const bool ok = e < hi;
            if (!__any(ok)) break; // (wave-uniform)
            int w = -1;
            bool first = false;
            if (ok) {
                w = out_col[e];
                if ((unsigned)w < (unsigned)g.n_int) {
                    const unsigned bit = 1u << (w & 31);
                    first = !(atomicOr(&ls.bits[w >> 5], bit) & bit);
                }
            }
            const unsigned long long firsts = __ballot(first);
            if (!firsts) continue;
            unsigned base = 0;
            if (lane_id() == 0) base = atomicAdd(&head->n_recv[b], (unsigned)__popcll(firsts));
            base = __shfl(base, 0, WAVE);
            if (first) {
                const unsigned at = base + (unsigned)__popcll(firsts & ((1ull << lane_id()) - 1ull));
                if (at < ls.list_cap) ls.recv[b][at] = w;
                else head->overflow = 1;
                const int len = g.row_ptr[w + 1] - g.row_ptr[w];
                edges += (unsigned long long)len;
                if (fw_row_long(len, piece)) {
                    const unsigned np = (unsigned)fw_pieces(len, piece);
                    const unsigned la = atomicAdd(&head->fw.n_long, 1u);
                    const unsigned ib = atomicAdd(&head->fw.n_items, np);
                    if (la >= long_cap || ib + np > item_cap) {
                        head->fw.overflow = 1;
                    } else {
                        FwLong lr;
                        lr.row = w;
                        lr.base = ib;
                        lr.np = np;
                        lr.pad = 0;
                        longs[la] = lr;
                        for (unsigned k = 0; k < np; ++k) items[ib + k] = fw_item((unsigned)w, k);
                    }
                }
            }
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) edges += __shfl_xor(edges, off, WAVE);
    if (edges && lane_id() == 0) atomicAdd(&head->work[2], edges);
}

// round k: r += the row sum over y[b], the short receivers. grid-stride over recv[b].
template <int PP, int LEVELS>
__global__ __launch_bounds__(FW_BLOCK) void k_fp_gather(FpHead *__restrict__ head, FwGraph g, const double *__restrict__ y, double *__restrict__ r,
                                                        int gw, int m, int T, int piece, FpLists ls, int b) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { // (the mark of this round is over)
        head->work[1] += head->n_recv[b];
        head->n_mark = 0;
    }
    const unsigned n = min(head->n_recv[b], ls.list_cap);
    const FwLane l = fw_lane(T);
    const int wave_rows = WAVE / (FW_SLOTS * T);
    const long long step = (long long)gridDim.x * FW_WAVES * wave_rows;
    for (long long t0 = ((long long)blockIdx.x * FW_WAVES + wave_id()) * wave_rows; t0 < n; t0 += step) { // (wave-uniform)
        const long long t = t0 + l.seg;
        if (t >= n) continue; // (no shuffle leaves a segment)
        const int u = ls.recv[b][t];
        if ((unsigned)u >= (unsigned)g.n_int) continue;
        const int r0 = g.row_ptr[u], r1 = g.row_ptr[u + 1];
        if (fw_row_long(r1 - r0, piece)) continue;
        const FwVal<PP> s = fw_walk<PP, LEVELS>(g, y, gw, l, r0, r1);
        if (l.slot == 0) {
#pragma unroll
            for (int q = 0; q < PP; ++q) {
                const int c0 = 2 * (l.pi + q * l.T);
                const size_t at = (size_t)u * gw + c0;
                if (c0 < m) r[at] = __dadd_rn(r[at], s.v[q].x);
                if (c0 + 1 < m) r[at + 1] = __dadd_rn(r[at + 1], s.v[q].y);
            }
        }
    }
}

// the long receivers of the round: a thread per (long row, column) adds the partials of k_fw_pieces as k_fw_long does
__global__ __launch_bounds__(FW_BLOCK) void k_fp_long(const FpHead *__restrict__ head, double *__restrict__ r, int gw, int m, int piece,
                                                      const FwLong *__restrict__ longs, unsigned long_cap, const double *__restrict__ pp) {
    if (head->fw.overflow) return;
    const long long total = (long long)min(head->fw.n_long, long_cap) * m;
    const int pb = fw_block_pieces(piece);
    for (long long j = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; j < total; j += (long long)gridDim.x * FW_BLOCK) {
        const FwLong lr = longs[j / m];
        const int c = (int)(j % m);
        const double *src = pp + (size_t)lr.base * gw + c;
        double acc = 0.0;
        for (unsigned b0 = 0; b0 < lr.np; b0 += (unsigned)pb) {
            FwCounter<1, FW_BLOCK_LEVELS> cnt;
            const int nb = (int)min((unsigned)pb, lr.np - b0);
            for (int k = 0; k < nb; ++k) {
                FwVal<1> v;
                v.v[0] = make_double2(src[(size_t)(b0 + k) * gw], 0.0);
                cnt.push(k, v);
            }
            const double B = cnt.close(nb).v[0].x;
            acc = b0 == 0 ? B : __dadd_rn(acc, B);
        }
        const size_t at = (size_t)lr.row * gw + c;
        r[at] = __dadd_rn(r[at], acc);
    }
}

// after the last round: a row above thr is a receiver of that round (recv[b])
template <bool SIGNED>
__global__ __launch_bounds__(FW_BLOCK) void k_fp_left(FpHead *__restrict__ head, FwGraph g, double eps, const double *__restrict__ r, int gw, int m,
                                                      FpLists ls, int b) {
    const unsigned n = min(head->n_recv[b], ls.list_cap);
    const long long step = (long long)gridDim.x * FW_BLOCK;
    for (long long i0 = (long long)blockIdx.x * FW_BLOCK + wave_id() * WAVE; i0 < n; i0 += step) { // (wave-uniform)
        const long long i = i0 + lane_id();
        unsigned mask = 0;
        if (i < n) {
            const int u = ls.recv[b][i];
            if ((unsigned)u < (unsigned)g.n_int) {
                const double thr = __dmul_rn(eps, (double)(g.out_row_ptr[u + 1] - g.out_row_ptr[u] + 1));
                for (int c = 0; c < m; ++c) {
                    const double rv = r[(size_t)u * gw + c];
                    if ((SIGNED ? fabs(rv) : rv) > thr) mask |= 1u << c;
                }
            }
        }
        if (!__any(mask != 0)) continue;
        for (int c = 0; c < m; ++c) {
            const unsigned long long in_c = __ballot((mask >> c) & 1u);
            if (in_c && lane_id() == 0) atomicAdd(&head->left[c], (unsigned long long)__popcll(in_c));
        }
    }
}

// p = 0.15 w at a seed without a row, in the dense copy
template <class T> __global__ void k_fp_poke(T *__restrict__ dst, long long at, double v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) dst[at] = (T)v;
}

} // namespace dppr
