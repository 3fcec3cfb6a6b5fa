// dppr_fcluster_plan.hpp -- what the full-length conductance sweep of a forward track (dppr_ftrack_cluster) decides before any
// device is involved: the argument checks, the offsets of the columns and the capacity rule, the tiles of the multi-tile prefix
// sum with their carries, the merge of two candidates for the best prefix, the pieces of a long row, and a plain host restatement
// of score -> order -> differences -> scan -> best over a small CSR that the kernels of dppr_fcluster.hpp must equal bit for bit.
// Pure host code without HIP includes (dppr_host_fcluster.hpp checks a call and lays it out with it, dppr_fcluster.hpp takes its
// constants; tests/native/fcluster_plan_test.cpp drives it on the CPU under the sanitizers).
//
// A CALL on the device:
//     1 load     the track's ext planes -> the planes of the forward family by internal id (k_ft_load)
//     2 count    a tile of FC_TILE external ids per workgroup: a 16-bit mask per id (bit c: column c qualifies), the tile's counts
//     3 scan     the tiles' counts -> the first position of every (tile, column); the counts come to the host ONCE
//     4 fill     (score bits, external id) of every qualifying vertex, per column, in ascending external id
//     5 sort     a stable descending radix sort of the 64-bit patterns per column (positive doubles order as their bits;
//                stability is the id tie rule); the order is the head L of it
//     6 rank     32-bit position per (live row, column), -1 where absent; ids and scores of the order to their outputs
//     7 rows     one wave per ordered vertex walks its out-row and its in-row; rows longer than the piece are queued in pieces
//     8 pieces   one wave per queued piece; 64-bit integer sums
//     9 scan     tile sums | a scan of the sums per column | apply: the prefix sums, phi and the tile's first minimum | the
//                column's first minimum over its tiles
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "dppr_query_plan.hpp"

namespace dppr {

static_assert(sizeof(dppr_fcluster_t) == 40, "five 8-byte fields");

constexpr int FC_TILE = 256;            // external ids per tile of the count / fill passes = threads of their workgroups
constexpr int FC_BLOCK = 256;           // every other kernel: four waves
constexpr int FC_WAVES = FC_BLOCK / 64; // ... one position (or one piece) each in the edge pass
constexpr int FC_SCAN_TILE = 1024;      // positions of a tile of the prefix sum (dppr_debug_ftrack_cluster: 64 .. 4096)
constexpr int FC_PIECE = 2048;          // entries of a row one wave walks; a longer row is cut into pieces of this many
constexpr int FC_HOOK_MIN = 64, FC_HOOK_MAX = 4096;

constexpr bool fc_hook_ok(int v) { return v == 0 || (v >= FC_HOOK_MIN && v <= FC_HOOK_MAX && (v & (v - 1)) == 0); }
constexpr int fc_scan_tile(int hook) { return hook ? hook : FC_SCAN_TILE; }
constexpr int fc_piece(int hook) { return hook ? hook : FC_PIECE; }

// the arguments that need no device and no track (min_score >= 0 is false for NaN)
inline bool fc_args_ok(int32_t order, double min_score, int64_t max_len, int64_t V, int32_t min_size, int64_t cap, int dest, const void *out_best,
                       const void *out_offsets, const void *ids, const void *score, const void *cut_out, const void *cut_in, const void *vol) {
    if (order != DPPR_FCLUSTER_BY_P && order != DPPR_FCLUSTER_BY_P_OVER_DEG) return false;
    if (!(min_score >= 0.0) || max_len < 0 || max_len > V || min_size < 1 || cap < 0) return false;
    if (dest != DPPR_DEST_HOST && dest != DPPR_DEST_DEVICE) return false;
    if (!out_best || !out_offsets) return false;
    return cap == 0 || ids || score || cut_out || cut_in || vol;
}

// no call can return more than one entry per (vertex, column): what a larger cap is worth to a destination
constexpr int64_t fc_cap_clamped(int64_t cap, int64_t V, int m) { return cap < V * (int64_t)m ? cap : V * (int64_t)m; }

// the score of a vertex: ONE division under BY_P_OVER_DEG
inline double fc_score(int32_t order, double p, int64_t outdeg) { return order == DPPR_FCLUSTER_BY_P_OVER_DEG ? p / (double)(outdeg + 1) : p; }
// a named vertex qualifies if score > min_score: false for a negative score, for +-0 (min_score >= 0) and for NaN
inline bool fc_qualifies(double score, double min_score, bool named) { return named && score > min_score; }

// length of a column's order and the offsets of the CSR over the columns
constexpr int64_t fc_len(int64_t qualifying, int64_t max_len) { return max_len == 0 || qualifying < max_len ? qualifying : max_len; }
struct FcCols {
    long long qoff[Q_LANES + 1]; // the qualifying entries of column c: [qoff[c], qoff[c + 1]) of the sort's arrays
    long long off[Q_LANES + 1];  // the order of column c: [off[c], off[c + 1]) of the outputs (entries past m repeat off[m])
    long long tile0[Q_LANES + 1]; // the scan tiles of column c: [tile0[c], tile0[c + 1])
    int m;
};
inline FcCols fc_cols(const long long *qualifying_offsets, int m, int64_t max_len, int scan_tile) {
    FcCols c{};
    c.m = m;
    for (int i = 0; i <= Q_LANES; ++i) {
        const int j = i < m ? i : m;
        c.qoff[i] = qualifying_offsets[j];
        if (i == 0) continue;
        const long long L = i <= m ? fc_len(qualifying_offsets[i] - qualifying_offsets[i - 1], max_len) : 0;
        c.off[i] = c.off[i - 1] + L;
        c.tile0[i] = c.tile0[i - 1] + (L + scan_tile - 1) / scan_tile;
    }
    return c;
}
// the capacity rule: the five arrays are written iff the entries fit
constexpr bool fc_fits(int64_t total, int64_t cap) { return total <= cap; }

// the block of the five arrays by position (T = off[m] entries), device and pinned host; every section 8-byte aligned
struct FcLayout {
    size_t off_ids = 0, off_score = 0, off_cut_out = 0, off_cut_in = 0, off_vol = 0;
    size_t total_bytes = 0;
};
constexpr FcLayout fc_layout(int64_t T) {
    FcLayout l;
    const size_t t = (size_t)(T > 0 ? T : 0);
    l.off_score = pad8(sizeof(int32_t) * t);
    l.off_cut_out = l.off_score + sizeof(double) * t;
    l.off_cut_in = l.off_cut_out + sizeof(int64_t) * t;
    l.off_vol = l.off_cut_in + sizeof(int64_t) * t;
    l.total_bytes = l.off_vol + sizeof(int64_t) * t;
    return l;
}
// the head of a call on the device: the qualifying offsets (17 x int64 and a word pair, as the sparse export's head), the control
// words of the piece list, the 16 records
constexpr size_t FC_HEAD_OFF_CTL = 8 * (Q_LANES + 1) + 8, FC_HEAD_OFF_BEST = FC_HEAD_OFF_CTL + 16;
constexpr size_t FC_HEAD_BYTES = FC_HEAD_OFF_BEST + sizeof(dppr_fcluster_t) * Q_LANES;

// pieces of a row of `len` entries walked in pieces (len > piece), and a bound on what a call can queue: a column's order holds a
// vertex once, so its split out-rows hold at most Ed entries and so do its split in-rows; a split row has < 2 len / piece pieces
constexpr long long fc_pieces(long long len, int piece) { return (len + piece - 1) / piece; }
constexpr size_t fc_list_cap(int m, long long Ed, int piece) { return (size_t)m * (size_t)(4 * (Ed / piece) + 4); }
struct FcItem { // a queued piece
    long long pos;  // absolute position in the outputs
    unsigned piece; // which piece of the row
    unsigned dir;   // 0: out-row, 1: in-row
};
static_assert(sizeof(FcItem) == 16, "two words");

// ---- the scan ------------------------------------------------------------------------------------------------------------------
struct FcSum { long long out, in, vol; };
constexpr FcSum fc_add(FcSum a, FcSum b) { return {a.out + b.out, a.in + b.in, a.vol + b.vol}; }

// a candidate for the best prefix: pos < 0 is "none". Ordered by (phi ascending, position ascending): the first minimum
struct FcBest {
    double phi;
    long long pos, cut, vol;
};
constexpr FcBest fc_none() { return {std::numeric_limits<double>::infinity(), -1, 0, 0}; }
inline bool fc_better(const FcBest &a, const FcBest &b) { // a before b?
    if (a.pos < 0) return false;
    if (b.pos < 0) return true;
    return a.phi < b.phi || (a.phi == b.phi && a.pos < b.pos);
}
inline FcBest fc_merge(const FcBest &a, const FcBest &b) { return fc_better(b, a) ? b : a; }
// position j (prefix sums cut, vol) as a candidate
inline FcBest fc_candidate(long long j, long long cut, long long vol, long long Ed, int min_size) {
    const long long den = vol < Ed - vol ? vol : Ed - vol;
    if (j + 1 < (long long)min_size || den <= 0) return fc_none();
    return {(double)cut / (double)den, j, cut, vol};
}
inline dppr_fcluster_t fc_record(long long L, const FcBest &b) {
    dppr_fcluster_t r;
    r.count = L;
    r.best_size = b.pos < 0 ? 0 : b.pos + 1;
    r.best_cut = b.pos < 0 ? 0 : b.cut;
    r.best_vol = b.pos < 0 ? 0 : b.vol;
    r.best_phi = b.pos < 0 ? std::numeric_limits<double>::infinity() : b.phi;
    return r;
}

// ---- the host restatement ----------------------------------------------------------------------------------------------------------
struct FcCsr { // the epoch by external id: out-rows with multiplicity
    int64_t V = 0;
    std::vector<int64_t> ptr; // [V + 1]
    std::vector<int32_t> col; // [Ed]
    int64_t edges() const { return ptr.empty() ? 0 : ptr.back(); }
};

struct FcResult {
    std::vector<int32_t> ids;
    std::vector<double> score;
    std::vector<int64_t> cut_out, cut_in, vol;
    dppr_fcluster_t best;
};

// One column as the device computes it: the qualifying entries in ascending id, a STABLE descending sort of the bit patterns, the
// per-position differences of dppr_cluster.hpp over both rows, the prefix sums tile by tile with carries, the tiles' first minima
// merged in order.
inline FcResult fc_host(const FcCsr &g, const double *p, int32_t order, double min_score, int64_t max_len, int32_t min_size, int scan_tile) {
    const int64_t V = g.V, Ed = g.edges();
    std::vector<int64_t> indeg((size_t)V, 0);
    for (int64_t e = 0; e < Ed; ++e) ++indeg[(size_t)g.col[(size_t)e]];
    struct Entry { uint64_t key; int32_t id; };
    std::vector<Entry> q;
    for (int64_t v = 0; v < V; ++v) {
        const int64_t deg = g.ptr[(size_t)v + 1] - g.ptr[(size_t)v];
        const double s = fc_score(order, p[v], deg);
        if (!fc_qualifies(s, min_score, deg > 0 || indeg[(size_t)v] > 0)) continue;
        uint64_t key;
        std::memcpy(&key, &s, 8);
        q.push_back({key, (int32_t)v});
    }
    std::stable_sort(q.begin(), q.end(), [](const Entry &a, const Entry &b) { return a.key > b.key; });
    const int64_t L = fc_len((int64_t)q.size(), max_len);
    FcResult r;
    std::vector<int64_t> rank((size_t)V, -1);
    for (int64_t j = 0; j < L; ++j) {
        r.ids.push_back(q[(size_t)j].id);
        double s;
        std::memcpy(&s, &q[(size_t)j].key, 8);
        r.score.push_back(s);
        rank[(size_t)q[(size_t)j].id] = j;
    }
    // differences: d_out[j] = #{out w: rho(w) > j} - #{in w: rho(w) < j}, d_in[j] = #{in w: rho(w) > j} - #{out w: rho(w) < j}
    std::vector<FcSum> d((size_t)L, FcSum{0, 0, 0});
    const int64_t absent = std::numeric_limits<int64_t>::max();
    for (int64_t u = 0; u < V; ++u)
        for (int64_t e = g.ptr[(size_t)u]; e < g.ptr[(size_t)u + 1]; ++e) {
            const int64_t w = g.col[(size_t)e];
            const int64_t ju = rank[(size_t)u] < 0 ? absent : rank[(size_t)u], jw = rank[(size_t)w] < 0 ? absent : rank[(size_t)w];
            if (ju != absent) { // u's out-row
                d[(size_t)ju].vol += 1;
                if (jw > ju) d[(size_t)ju].out += 1;
                if (jw < ju) d[(size_t)ju].in -= 1;
            }
            if (jw != absent) { // w's in-row
                if (ju > jw) d[(size_t)jw].in += 1;
                if (ju < jw) d[(size_t)jw].out -= 1;
            }
        }
    // the scan: tile sums, the exclusive scan of the sums, apply
    const int64_t tiles = (L + scan_tile - 1) / scan_tile;
    std::vector<FcSum> carry((size_t)tiles + 1, FcSum{0, 0, 0});
    for (int64_t t = 0; t < tiles; ++t) {
        FcSum s{0, 0, 0};
        for (int64_t j = t * scan_tile; j < std::min<int64_t>(L, (t + 1) * scan_tile); ++j) s = fc_add(s, d[(size_t)j]);
        carry[(size_t)t + 1] = fc_add(carry[(size_t)t], s);
    }
    FcBest best = fc_none();
    r.cut_out.resize((size_t)L);
    r.cut_in.resize((size_t)L);
    r.vol.resize((size_t)L);
    for (int64_t t = 0; t < tiles; ++t) {
        FcSum s = carry[(size_t)t];
        FcBest tb = fc_none();
        for (int64_t j = t * scan_tile; j < std::min<int64_t>(L, (t + 1) * scan_tile); ++j) {
            s = fc_add(s, d[(size_t)j]);
            r.cut_out[(size_t)j] = s.out;
            r.cut_in[(size_t)j] = s.in;
            r.vol[(size_t)j] = s.vol;
            tb = fc_merge(tb, fc_candidate(j, s.out, s.vol, Ed, min_size));
        }
        best = fc_merge(best, tb);
    }
    r.best = fc_record(L, best);
    return r;
}

} // namespace dppr
