// dppr_ftrack.hpp -- the forward track (dppr_ftrack_*): the push state (p, r) of up to 16 weighted start sets kept by EXTERNAL id and
// moved from epoch k to epoch k + 1 by a fix-up over the batch's records and the signed rounds of dppr_fpush.hpp. Never called from
// the update path; no state of the solver is read or written, no field of an Epoch is written. include/dppr.h states every
// rounding; dppr_ftrack_plan.hpp has the steps of a call and a host restatement.
//
// STATE   sp | sr, each [V][gw] doubles by external id (FTrack::state). A call works on the planes of the forward family by internal
//         id (p | r | y0 | y1): k_ft_load copies every vertex that has an id (live or parked) in, k_ft_store copies it back and
//         leaves |r| in y0 for the fold of rem (k_fw_rem). A vertex without an id keeps what the ext planes hold.
// FIX-UP  the records' (tail, index) and (head, index) pairs sorted by the device radix sort (stable: a run holds its records in
//         batch order). k_ft_tails, a thread per (sorted position, column): the thread at the start of a tail's run counts the run's
//         inserts and deletes, takes d1 from the epoch's out-CSR, changes p and r of the tail in its column and stores c for every
//         record of the run. k_ft_heads, after it: the thread at the start of a head's run adds its records' c in batch order.
//         A value of p or r is written by the one thread that owns (vertex, column) in that launch; the counters of `fix` and the
//         candidate list are integer sums and a set: where a row stands in the list enters no value. No floating-point atomic.
// ROUNDS  k_fp_select<true> / k_fp_left<true>: |r| > thr. The candidates of round 1 are the records' tails and heads (entered by the
//         two kernels above) when every column was converged before the fix-up, else the rows k_ft_scan finds above thr.
// DESIGN.md section 9t has the resource usage and the measurement.
#pragma once

#include "dppr_fpush.hpp"
#include "dppr_ftrack_plan.hpp"

namespace dppr {

// a row enters the candidates of round 1 (recv[0]) once
__device__ __forceinline__ void ft_enter(FpHead *__restrict__ head, const FpLists &ls, int row) {
    const unsigned bit = 1u << (row & 31);
    if (!(atomicOr(&ls.bits[row >> 5], bit) & bit)) {
        const unsigned at = atomicAdd(&head->n_recv[0], 1u);
        if (at < ls.list_cap) ls.recv[0][at] = row;
        else head->overflow = 1;
    }
}

// grid-stride over [V][gw]: the ext planes into the rows of every vertex with an id
__global__ __launch_bounds__(FW_BLOCK) void k_ft_load(const double *__restrict__ sp, const double *__restrict__ sr, const int *__restrict__ ext2int,
                                                      int V, int gw, double *__restrict__ p, double *__restrict__ r) {
    const long long total = (long long)V * gw;
    for (long long t = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * FW_BLOCK) {
        const int row = ext2int[t / gw];
        if ((unsigned)row >= (unsigned)V) continue;
        const size_t at = (size_t)row * gw + (size_t)(t % gw);
        p[at] = sp[t];
        r[at] = sr[t];
    }
}

// ... and back; |r| by internal id into `ra` (a y plane: the rounds are over)
__global__ __launch_bounds__(FW_BLOCK) void k_ft_store(const double *__restrict__ p, const double *__restrict__ r, const int *__restrict__ ext2int,
                                                       int V, int gw, double *__restrict__ sp, double *__restrict__ sr, double *__restrict__ ra) {
    const long long total = (long long)V * gw;
    for (long long t = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * FW_BLOCK) {
        const int row = ext2int[t / gw];
        if ((unsigned)row >= (unsigned)V) continue;
        const size_t at = (size_t)row * gw + (size_t)(t % gw);
        const double rv = r[at];
        if (sp) {
            sp[t] = p[at];
            sr[t] = rv;
        }
        ra[at] = fabs(rv);
    }
}

// the sort's input: keys = tails | heads, values = the record index
__global__ __launch_bounds__(FW_BLOCK) void k_ft_keys(const int *__restrict__ b1, const int *__restrict__ b2, int L, uint32_t *__restrict__ kt,
                                                      uint32_t *__restrict__ kh, uint32_t *__restrict__ idx) {
    for (int i = blockIdx.x * FW_BLOCK + threadIdx.x; i < L; i += gridDim.x * FW_BLOCK) {
        kt[i] = (uint32_t)b1[i];
        kh[i] = (uint32_t)b2[i];
        idx[i] = (uint32_t)i;
    }
}

// step T. st / sv: the records sorted by tail (tail, record index). cr [L][gw]: c by record.
__global__ __launch_bounds__(FW_BLOCK) void k_ft_tails(FpHead *__restrict__ head, FwGraph g, const uint32_t *__restrict__ st,
                                                       const uint32_t *__restrict__ sv, const uint8_t *__restrict__ ins, int L, double *__restrict__ p,
                                                       double *__restrict__ r, int gw, int m, double *__restrict__ cr, FpLists ls, int enter,
                                                       unsigned long long *__restrict__ fix) {
    const long long total = (long long)L * m;
    for (long long t = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * FW_BLOCK) {
        const int j = (int)(t / m), c = (int)(t % m);
        const uint32_t u = st[j];
        if (j > 0 && st[j - 1] == u) continue; // (the thread at the start of the run does the run)
        if (u >= (unsigned)g.n_int) continue;  // (a record names live rows: never)
        int n_ins = 0, n_del = 0, end = j;
        for (; end < L && st[end] == u; ++end) {
            const uint32_t i = sv[end];
            if (i < (uint32_t)L && ins[i]) ++n_ins;
            else ++n_del;
        }
        const int d1 = g.out_row_ptr[u + 1] - g.out_row_ptr[u], d0 = d1 - n_ins + n_del;
        const size_t at = (size_t)u * gw + c;
        const double den0 = (double)(d0 + 1), pv = p[at];
        const double gv = __ddiv_rn(pv, __dmul_rn(FW_ALPHA, den0)), cv = __dmul_rn(FW_DAMP, gv);
        if (d1 != d0) {
            p[at] = __ddiv_rn(__dmul_rn(pv, (double)(d1 + 1)), den0);
            r[at] = __dsub_rn(r[at], __dmul_rn((double)(d1 - d0), gv));
        }
        for (int k = j; k < end; ++k) {
            const uint32_t i = sv[k];
            if (i < (uint32_t)L) cr[(size_t)i * gw + c] = cv;
        }
        if (c == 0) {
            atomicAdd(&fix[1], 1ull);
            if (enter) ft_enter(head, ls, (int)u);
        }
    }
}

// step H. sh / sv: the records sorted by head (head, record index): a run holds its records in batch order.
__global__ __launch_bounds__(FW_BLOCK) void k_ft_heads(FpHead *__restrict__ head, FwGraph g, const uint32_t *__restrict__ sh,
                                                       const uint32_t *__restrict__ sv, const uint8_t *__restrict__ ins, int L, double *__restrict__ r,
                                                       int gw, int m, const double *__restrict__ cr, FpLists ls, int enter,
                                                       unsigned long long *__restrict__ fix) {
    const long long total = (long long)L * m;
    for (long long t = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * FW_BLOCK) {
        const int j = (int)(t / m), c = (int)(t % m);
        const uint32_t w = sh[j];
        if (j > 0 && sh[j - 1] == w) continue;
        if (w >= (unsigned)g.n_int) continue; // (never)
        const size_t at = (size_t)w * gw + c;
        double x = r[at];
        for (int k = j; k < L && sh[k] == w; ++k) {
            const uint32_t i = sv[k];
            if (i >= (uint32_t)L) continue; // (never)
            const double cv = cr[(size_t)i * gw + c];
            x = ins[i] ? __dadd_rn(x, cv) : __dsub_rn(x, cv);
        }
        r[at] = x;
        if (c == 0) {
            atomicAdd(&fix[2], 1ull);
            if (enter) ft_enter(head, ls, (int)w);
        }
    }
}

// the candidates of round 1 by one scan: the live rows with |r| > thr in any column
__global__ __launch_bounds__(FW_BLOCK) void k_ft_scan(FpHead *__restrict__ head, FwGraph g, double eps, const double *__restrict__ r, int gw, int m,
                                                      FpLists ls) {
    for (long long u = (long long)blockIdx.x * FW_BLOCK + threadIdx.x; u < g.n_int; u += (long long)gridDim.x * FW_BLOCK) {
        const double thr = __dmul_rn(eps, (double)(g.out_row_ptr[u + 1] - g.out_row_ptr[u] + 1));
        bool any = false;
        for (int c = 0; c < m; ++c) any = any || fabs(r[(size_t)u * gw + c]) > thr;
        if (any) ft_enter(head, ls, (int)u);
    }
}

} // namespace dppr
