// dppr_subgraph_plan.hpp -- what the induced subgraph of a top-k order (dppr_subgraph / dppr_group_subgraph) decides before any
// device is involved: the argument check, the sizes of its workspace, the block of a host destination with which part of it a call
// copies back, which kernel fills a row, and THE rule for a row, subgraph_row, a plain restatement of include/dppr.h that the fill
// kernels of dppr_subgraph.hpp must equal entry for entry. Pure host code without HIP includes (dppr_host_query.hpp checks a call
// and lays its block out with it; tests/native/subgraph_plan_test.cpp drives it on the CPU).
//
// BLOCK of a call on the device:
//     [offsets 17 x int64][counts 16 x int32]  <- SG_HEAD_BYTES = 200, always copied back, BEFORE the fill: the host decides
//     [ids n x k, padded to 8 bytes][p n x k][row_ptr n x (k + 1)][col cap x int32: a host destination alone]
// A device destination writes ids, p, row_ptr and col in place; a section whose pointer is NULL is still written, into the block
// (the fill reads row_ptr, the rank table ids). A host destination copies the sections from the first to the last one asked for.
#pragma once

#include "dppr_cluster_plan.hpp"

namespace dppr {

static_assert(DPPR_SUBGRAPH_MAX == DPPR_TOPK_MAX, "the subgraph is induced by the order dppr_topk defines");
static_assert(DPPR_SUBGRAPH_MAX < CL_ABSENT, "every position is below the rank of a vertex outside the order");

constexpr int SG_WAVE_CAP = 256;      // matched entries of a row one wave can place (its keys lie in LDS: 1 KiB per wave)
constexpr int SG_WAVE_MAX = 256;      // ... and the most it is given by default (measured, DESIGN.md 9i: up to the cap a wave is no slower than the
                                      // histogram kernel and takes a sixteenth of its threads): above, the row goes to the histogram kernel
constexpr int SG_LONG_BLOCK = 1024;   // k_sg_long: one workgroup per row, a histogram over the positions in LDS
constexpr int SG_PER_THREAD = DPPR_SUBGRAPH_MAX / SG_LONG_BLOCK; // consecutive bins of a thread of its scan
constexpr int SG_LONG_GRID = 256;     // ... from a fixed grid over the rows queued for it

struct SgHead {
    long long offsets[Q_LANES + 1]; // offsets[i] .. offsets[i + 1]: source i; entries past n repeat offsets[n]
    int count[Q_LANES];             // L of every source
};
constexpr size_t SG_HEAD_BYTES = 8 * (Q_LANES + 1) + 4 * Q_LANES;
static_assert(sizeof(SgHead) == SG_HEAD_BYTES && SG_HEAD_BYTES % 8 == 0, "the head of the block is 17 offsets and 16 counts");

// the arguments that need no device: k, min_p >= 0 (false for NaN), cap >= 0, a known dest, the two host arrays, col wherever
// something could be written
inline bool subgraph_args_ok(int32_t k, double min_p, int64_t cap, int dest, const void *offsets, const void *counts, const void *col) {
    if (k < 1 || k > DPPR_SUBGRAPH_MAX || !(min_p >= 0.0) || cap < 0) return false;
    if ((dest != DPPR_DEST_HOST && dest != DPPR_DEST_DEVICE) || !offsets || !counts) return false;
    return cap == 0 || col;
}

// no call can return more than one entry per (stored edge, source): what a larger cap is worth to the block and to the range of
// a device destination that is checked
constexpr int64_t sg_cap_clamped(int64_t cap, int64_t Ed, int n) { return cap < Ed * (int64_t)n ? cap : Ed * (int64_t)n; }

// ints of the per-position work: the control words (4), the matches of every position [n][k], the rows queued for k_sg_long [n][k]
constexpr size_t sg_work_elems(int n, int k) { return 4 + 2 * (size_t)n * (size_t)k; }

// bytes of the sections a device destination must hold
constexpr size_t sg_ids_bytes(int n, int k) { return sizeof(int32_t) * (size_t)n * (size_t)k; }
constexpr size_t sg_p_bytes(int n, int k) { return sizeof(double) * (size_t)n * (size_t)k; }
constexpr size_t sg_row_ptr_bytes(int n, int k) { return sizeof(int64_t) * (size_t)n * ((size_t)k + 1); }
constexpr size_t sg_col_bytes(int64_t cap) { return sizeof(int32_t) * (size_t)(cap > 0 ? cap : 0); }

struct SgLayout {
    size_t off_head = 0, off_ids = SG_HEAD_BYTES, off_p = 0, off_row_ptr = 0, off_col = 0;
    size_t total_bytes = 0;            // the block on the device
    size_t copy_lo = 0, copy_hi = 0;   // [copy_lo, copy_hi): what a host destination copies back after the head (empty: nothing)
};

// cap: entries of col the block stages (a host destination, clamped; 0 for a device destination and for the size query)
constexpr SgLayout sg_layout(int n, int k, int64_t cap, bool ids, bool p, bool row_ptr, bool col) {
    SgLayout l;
    l.off_p = l.off_ids + pad8(sg_ids_bytes(n, k));
    l.off_row_ptr = l.off_p + sg_p_bytes(n, k);
    l.off_col = l.off_row_ptr + sg_row_ptr_bytes(n, k);
    l.total_bytes = l.off_col + pad8(sg_col_bytes(cap));
    const bool c = col && cap > 0;
    l.copy_lo = ids ? l.off_ids : p ? l.off_p : row_ptr ? l.off_row_ptr : c ? l.off_col : l.total_bytes;
    l.copy_hi = c ? l.off_col + sg_col_bytes(cap) : row_ptr ? l.off_col : p ? l.off_row_ptr : ids ? l.off_p : l.total_bytes;
    if (l.copy_hi < l.copy_lo) l.copy_hi = l.copy_lo;
    return l;
}

// which kernel fills a row of `len` stored entries of which `matched` lie in the order: the wave that owns the position, or the
// histogram kernel (a row the count pass walked in chunks, or more matches than a wave is given)
constexpr bool sg_row_is_long(long long len, long long matched, int wave_max) { return len > CL_SPLIT || matched > wave_max; }
constexpr bool sg_wave_max_ok(int wave_max) { return wave_max >= 0 && wave_max <= SG_WAVE_CAP; }

// slot of entry t among the m matched entries of a row placed by a wave: the number of smaller (position, entry index) pairs
inline int sg_slot(const int32_t *key, int m, int t) {
    int r = 0;
    for (int u = 0; u < m; ++u) r += (key[u] < key[t] || (key[u] == key[t] && u < t)) ? 1 : 0;
    return r;
}

// THE rule for a row (include/dppr.h): the positions of the heads of a vertex's stored out-edges that lie in the order, ascending,
// a position as often as it is stored. heads [len]: the row in any order; pos [V]: position of every vertex, -1 outside the order;
// out [at least the returned count]. Returns the number of entries written.
inline int64_t subgraph_row(const int32_t *heads, int64_t len, const int32_t *pos, int32_t L, int32_t *out) {
    int64_t m = 0;
    for (int32_t want = 0; want < L; ++want) // (quadratic on purpose: nothing but the definition)
        for (int64_t e = 0; e < len; ++e)
            if (pos[heads[e]] == want) out[m++] = want;
    return m;
}

} // namespace dppr
