// dppr_cluster_plan.hpp -- what the conductance sweep over a top-k order (dppr_cluster / dppr_group_cluster) decides before any
// device is involved: the argument check, the sizes of its workspace, the result block with which part of it a call copies back,
// and THE rule for the best prefix, cluster_best, a plain restatement of include/dppr.h that k_cl_scan of dppr_cluster.hpp must
// equal bit for bit. Pure host code without HIP includes (dppr_host_query.hpp checks a call and lays its block out with it;
// tests/native/cluster_plan_test.cpp drives it on the CPU).
//
// BLOCK of a call, one copy to the host:
//     [16 dppr_cluster_t] <- CL_OFF_IDS = 512 bytes   [ids n x k, padded to 8 bytes][cut_out n x k][cut_in n x k][vol n x k]
// Every section is always written on the device; the copy ends with the last section the caller asked for (all four NULL: the
// 512 bytes of the records alone).
#pragma once

#include <limits>

#include "dppr_query_plan.hpp"

namespace dppr {

static_assert(DPPR_CLUSTER_MAX == DPPR_TOPK_MAX, "the sweep walks the order dppr_topk defines");
static_assert(sizeof(dppr_cluster_t) == 32, "the block holds 16 records of 32 bytes");

constexpr int CL_SPLIT = 2048;          // entries of a row one wave walks; a longer row is cut into chunks of this many
constexpr int CL_ABSENT = 0xffff;       // rank of a vertex outside the order: above every rank (ranks are < 8192)
constexpr int CL_BLOCK = 256;           // k_cl_rank / k_cl_rows / k_cl_big: four waves
constexpr int CL_WAVES = CL_BLOCK / 64; // ... one position (or one chunk) each
constexpr int CL_SCAN_BLOCK = 1024;     // k_cl_scan: one workgroup per lane
constexpr int CL_PER_THREAD = DPPR_CLUSTER_MAX / CL_SCAN_BLOCK; // consecutive positions of a thread of the scan
constexpr size_t CL_OFF_IDS = sizeof(dppr_cluster_t) * (size_t)Q_LANES;

inline bool cluster_args_ok(int32_t k, double min_p, int32_t min_size, const void *out_best) {
    return k >= 1 && k <= DPPR_CLUSTER_MAX && min_p >= 0.0 && min_size >= 1 && min_size <= k && out_best; // (min_p >= 0 is false for NaN)
}

// entries of a rank table row: the lanes rounded up to a power of two (a row is 2, 4, .. 32 bytes and never straddles a line)
constexpr int cl_stride(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16; }
constexpr size_t cl_rank_elems(size_t rows, int n) { return (rows > 0 ? rows : 1) * (size_t)cl_stride(n); }
// chunks of a row of `len` entries that is walked by chunks (len > CL_SPLIT)
constexpr long long cl_chunks(long long len) { return (len + CL_SPLIT - 1) / CL_SPLIT; }
// chunk items a call can queue. A lane's order holds a vertex once, so its split out-rows hold at most Ed entries and so do its
// split in-rows; a split row of len entries has cl_chunks(len) < 2 len / CL_SPLIT chunks.
constexpr size_t cl_list_cap(int n, long long Ed) { return (size_t)n * (size_t)(4 * (Ed / CL_SPLIT) + 4); }
// a chunk item: position (lane * k + j) | direction (0: out-row, 1: in-row) | chunk number
constexpr unsigned long long cl_item(unsigned pos, unsigned dir, unsigned chunk) {
    return ((unsigned long long)pos << 32) | ((unsigned long long)dir << 31) | chunk;
}
constexpr unsigned cl_item_pos(unsigned long long it) { return (unsigned)(it >> 32); }
constexpr unsigned cl_item_dir(unsigned long long it) { return (unsigned)(it >> 31) & 1u; }
constexpr unsigned cl_item_chunk(unsigned long long it) { return (unsigned)it & 0x7fffffffu; }

struct ClLayout {
    size_t off_best = 0, off_ids = CL_OFF_IDS, off_cut_out = 0, off_cut_in = 0, off_vol = 0;
    size_t copy_bytes = 0;  // what comes back to the host
    size_t total_bytes = 0; // the block on the device
};

constexpr ClLayout cl_layout(int n, int k, bool ids, bool cut_out, bool cut_in, bool vol) {
    ClLayout l;
    const size_t nk = (size_t)n * (size_t)k;
    l.off_cut_out = l.off_ids + pad8(sizeof(int32_t) * nk);
    l.off_cut_in = l.off_cut_out + sizeof(int64_t) * nk;
    l.off_vol = l.off_cut_in + sizeof(int64_t) * nk;
    l.total_bytes = l.off_vol + sizeof(int64_t) * nk;
    l.copy_bytes = vol ? l.total_bytes : cut_in ? l.off_vol : cut_out ? l.off_cut_in : ids ? l.off_cut_out : l.off_ids;
    return l;
}

// The best prefix of an order of L vertices (include/dppr.h): den[j] = min(vol[j], Ed - vol[j]); prefix j is eligible if
// j + 1 >= min_size and den[j] > 0; phi[j] = (double)cut_out[j] / (double)den[j]; the smallest phi wins, the smallest j among equals.
inline dppr_cluster_t cluster_best(const int64_t *cut_out, const int64_t *vol, int32_t L, int64_t Ed, int32_t min_size) {
    dppr_cluster_t b;
    b.count = L;
    b.best_size = 0;
    b.best_cut = 0;
    b.best_vol = 0;
    b.best_phi = std::numeric_limits<double>::infinity();
    for (int32_t j = 0; j < L; ++j) {
        const int64_t den = vol[j] < Ed - vol[j] ? vol[j] : Ed - vol[j];
        if (j + 1 < min_size || den <= 0) continue;
        const double phi = (double)cut_out[j] / (double)den;
        if (b.best_size == 0 || phi < b.best_phi) {
            b.best_size = j + 1;
            b.best_cut = cut_out[j];
            b.best_vol = vol[j];
            b.best_phi = phi;
        }
    }
    return b;
}

} // namespace dppr
