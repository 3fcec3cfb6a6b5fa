// dppr_forward_plan.hpp -- what the forward sweep (dppr_forward) decides before any device is involved: the limits and the
// rejections, which parts of dppr_forward_out_t a call asks for, the check schedule (after the iterations 8, 16, .. and after
// the last), the shape of the gather (the team that shares a gathered row, the segment that shares an in-row, the pieces a long
// in-row is cut into with the bounds of their lists), the grids, the work space, and a plain host restatement of a row's sum
// exactly as the device forms it. Pure host code without HIP includes (dppr_host_query.hpp checks a call and lays it out with it,
// dppr_forward.hpp takes its constants and its arithmetic; tests/native/forward_plan_test.cpp drives it on the CPU under the
// sanitizers).
//
// THE ROW SUM is the fold of include/dppr.h (dppr_dot_plan.hpp: dot_fold_ref) over the terms of an in-row in stored order. The
// device realises that one tree in aligned pieces, each a power of two of the one below:
//     round    FW_SLOTS = 8 entries        the 8 slots of a segment meet by a butterfly (xor T, 2T, 4T: + commutes)
//     piece    2^j rounds, <= `piece`      a binary counter of partial sums (FwCounter): the left operand is always the earlier
//     block    2^16 / piece pieces         the same counter over the pieces' partials (a LONG row only)
//     row      the blocks in ascending order
// A level that is missing at the end is padding: every term is >= +0.0, x + +0.0 = x, so the counter is closed by adding its
// occupied levels from the lowest up and the result has the bits of the padded tree.
#pragma once

#include <vector>

#include "dppr_dot_plan.hpp"
#include "dppr_export_plan.hpp"
#include "dppr_query_plan.hpp"

namespace dppr {

constexpr int FW_BLOCK = 256;                 // every kernel of dppr_forward.hpp: four waves
constexpr int FW_WAVES = FW_BLOCK / 64;
constexpr int FW_SLOTS = 8;                   // entries of an in-row a segment takes per round
constexpr int FW_PIECE = 512;                 // entries of a piece (dppr_debug_forward changes it)
constexpr int FW_PIECE_MIN = 64, FW_PIECE_MAX = 4096;
constexpr int FW_LEVELS_SHORT = 7;            // counter levels of a piece of <= FW_PIECE entries: 64 rounds fill level 6
constexpr int FW_LEVELS_LONG = 10;            // ... of <= FW_PIECE_MAX entries: 512 rounds fill level 9
constexpr int FW_BLOCK_LEVELS = 11;           // counter levels over the pieces of a block: 2^16 / FW_PIECE_MIN = 1024 fill level 10
constexpr int FW_GRID_MAX = 16384;
static_assert((FW_PIECE / FW_SLOTS) == (1 << (FW_LEVELS_SHORT - 1)) && (FW_PIECE_MAX / FW_SLOTS) == (1 << (FW_LEVELS_LONG - 1)) &&
                  (DOT_BLOCK / FW_PIECE_MIN) == (1 << (FW_BLOCK_LEVELS - 1)),
              "a full piece / a full block fills the top level of its counter");
static_assert(DPPR_FORWARD_MAX_M == Q_LANES && DPPR_FORWARD_CHECK == 8, "the columns are the lanes of a group's row");

constexpr double FW_ALPHA = 0.15, FW_DAMP = 0.85; // (the literals of the contract; 1.0 - 0.15 rounds to the same double as 0.85)

// ---- the call ------------------------------------------------------------------------------------------------------------------
enum : uint32_t { FW_META = 1u << 0, FW_TOPK = 1u << 1, FW_AT = 1u << 2, FW_DENSE = 1u << 3 };

// the parts a call asks for: a part is asked for when any of its pointers is not NULL
inline uint32_t fw_which(const dppr_forward_out_t *o) {
    if (!o) return 0;
    uint32_t w = 0;
    if (o->iters_used || o->rem) w |= FW_META;
    if (o->topk_ids || o->topk_f || o->topk_counts) w |= FW_TOPK;
    if (o->at_ids || o->at_f) w |= FW_AT;
    if (o->dense_dev) w |= FW_DENSE;
    return w;
}
// tol >= 0 is false for a NaN; an infinite tol is refused too
inline bool fw_args_ok(const int32_t *starts, int32_t m, int32_t iters, double tol, const dppr_forward_out_t *out) {
    return starts && out && m >= 1 && m <= DPPR_FORWARD_MAX_M && iters >= 1 && iters <= DPPR_FORWARD_MAX_ITERS && tol >= 0.0 &&
           std::isfinite(tol);
}
// the parts asked for are complete (the ids of the at part and the device pointer of the dense part are checked by the caller)
inline bool fw_parts_ok(const dppr_forward_out_t *o) {
    const uint32_t w = fw_which(o);
    if ((w & FW_TOPK) && !topk_args_ok(o->k, o->min_f, o->topk_ids, o->topk_f, o->topk_counts)) return false;
    if ((w & FW_AT) && !(o->at_ids && o->at_f && o->n_at >= 1 && o->n_at <= DPPR_FORWARD_AT_MAX)) return false;
    if ((w & FW_DENSE) && !ex_dense_args_ok(DPPR_DENSE_P, o->dense_dtype, o->dense_layout)) return false;
    return true;
}

// ---- the check schedule --------------------------------------------------------------------------------------------------------
// rem is evaluated after iteration k (1-based) when ...
constexpr bool fw_is_check(int k, int iters) { return k == iters || (k < iters && k % DPPR_FORWARD_CHECK == 0); }
// the first check after iteration k (k < iters)
constexpr int fw_next_check(int k, int iters) {
    const int nxt = (k / DPPR_FORWARD_CHECK + 1) * DPPR_FORWARD_CHECK;
    return nxt < iters ? nxt : iters;
}
// what a start without a row reports
constexpr int fw_rowless_iters(int iters) { return iters < DPPR_FORWARD_CHECK ? iters : DPPR_FORWARD_CHECK; }

// ---- the shape of the gather -----------------------------------------------------------------------------------------------------
// row width of m columns: that of a group of m sources (dppr_multi.hpp row_width; asserted equal in dppr_forward.hpp)
constexpr int fw_row_width(int m) { return m <= 2 ? 2 : (m + 1) / 2 * 2; }
// 16-byte pieces of a row
constexpr int fw_row_pieces(int gw) { return gw / 2; }
constexpr int fw_pow2_ceil(int x) {
    int p = 1;
    while (p < x) p *= 2;
    return p;
}
// lanes of a team (one gathered row): the plan's choice is one lane per 16-byte piece, rounded up to a power of two; a lane
// takes at most two pieces (piece pi and pi + T), so a forced team is raised to half the pieces
constexpr int fw_team_min(int gw) { return fw_pow2_ceil((fw_row_pieces(gw) + 1) / 2); }
constexpr int fw_team(int gw, int forced) {
    const int t = forced > 0 ? forced : fw_pow2_ceil(fw_row_pieces(gw));
    return t < fw_team_min(gw) ? fw_team_min(gw) : t;
}
// pieces of a row per lane of the team: 1 or 2
constexpr int fw_lane_pieces(int gw, int team) { return (fw_row_pieces(gw) + team - 1) / team; }
// lanes of a segment (one in-row at a time): FW_SLOTS teams; in-rows that share a wave
constexpr int fw_segment(int team) { return FW_SLOTS * team; }
constexpr int fw_wave_rows(int team) { return 64 / fw_segment(team); }
inline bool fw_hook_ok(int piece_edges, int team) {
    const bool p_ok = piece_edges == 0 || (piece_edges >= FW_PIECE_MIN && piece_edges <= FW_PIECE_MAX && (piece_edges & (piece_edges - 1)) == 0);
    return p_ok && (team == 0 || team == 1 || team == 2 || team == 4 || team == 8);
}
constexpr int fw_piece(int forced) { return forced > 0 ? forced : FW_PIECE; }
constexpr int fw_levels(int piece) { return piece <= FW_PIECE ? FW_LEVELS_SHORT : FW_LEVELS_LONG; }

// ---- the pieces of a long in-row -------------------------------------------------------------------------------------------------
constexpr bool fw_row_long(long long len, int piece) { return len > piece; }
constexpr long long fw_pieces(long long len, int piece) { return len <= 0 ? 0 : (len + piece - 1) / piece; }
constexpr long long fw_piece_lo(int piece, long long k) { return k * piece; }
constexpr long long fw_piece_hi(long long len, int piece, long long k) { return (k + 1) * piece < len ? (k + 1) * piece : len; }
// pieces of a block of the fold
constexpr int fw_block_pieces(int piece) { return (int)(DOT_BLOCK / piece); }
// Pieces the long rows of a graph of Ed entries can queue: a long row has len > piece, so its ceil(len / piece) pieces are fewer
// than 2 len / piece, and the long rows together hold at most Ed entries. Long rows: fewer than Ed / piece + 1.
constexpr size_t fw_item_cap(long long Ed, int piece) { return (size_t)(2 * (Ed / piece) + 2); }
constexpr size_t fw_long_cap(long long Ed, int piece) { return (size_t)(Ed / piece + 1); }
struct FwLong { // a long row: its internal id, its first queued piece and how many follow
    int row;
    unsigned base, np, pad;
};
static_assert(sizeof(FwLong) == 16, "a long row of the list is 16 bytes");
// a queued piece: row (internal id) << 32 | piece number
constexpr unsigned long long fw_item(unsigned row, unsigned k) { return ((unsigned long long)row << 32) | k; }
constexpr unsigned fw_item_row(unsigned long long it) { return (unsigned)(it >> 32); }
constexpr unsigned fw_item_piece(unsigned long long it) { return (unsigned)it; }

// ---- the grids -------------------------------------------------------------------------------------------------------------------
constexpr int fw_units_grid(long long units, int team) {
    const long long per_wg = (long long)FW_WAVES * fw_wave_rows(team);
    const long long g = (units + per_wg - 1) / per_wg;
    return g < 1 ? 1 : g < FW_GRID_MAX ? (int)g : FW_GRID_MAX;
}
constexpr int fw_rem_grid(int64_t V) {
    const int64_t tiles = dot_tiles(V);
    return tiles < 1 ? 1 : tiles < 2048 ? (int)tiles : 2048;
}

// ---- the work space on the device ------------------------------------------------------------------------------------------------
struct FwHead {                    // zeroed per call, then the starts are copied in
    unsigned frozen;               // bit c: column c takes no further part (THE word the host reads back per chunk)
    unsigned n_items, n_long;      // queued pieces, long rows
    unsigned overflow;             // a list was too short (fw_item_cap / fw_long_cap: never)
    int iters_used[Q_LANES];
    double rem[Q_LANES];           // as frozen
    double cur[Q_LANES];           // the fold of the last check
    int starts[Q_LANES];           // external ids
    int rowless[Q_LANES];          // 1: the start has no row (answered by the host)
    DotHead dot;                   // (never raised: k_dot_combine reads it)
};
// doubles of the four planes y | y' | f | x, each [V][gw]
constexpr size_t fw_plane_elems(int64_t V, int gw) { return (size_t)(V > 0 ? V : 1) * (size_t)gw; }
// doubles of the dot family's partials the rem fold takes: [m][whole blocks of tiles]
constexpr long long fw_part_stride(int64_t V) { return dot_cols(V) > 0 ? dot_cols(V) : DOT_TPB; }
constexpr size_t fw_part_elems(int64_t V, int m) { return (size_t)m * (size_t)fw_part_stride(V); }
constexpr unsigned fw_all(int m) { return m >= 32 ? ~0u : (1u << m) - 1u; }

// ---- the row sum as the device forms it, on the host -----------------------------------------------------------------------------
// (volatile: every sum is rounded to double where it stands)
inline double fw_add(double a, double b) {
    volatile double s = a + b;
    return s;
}
// a binary counter of partial sums over items pushed in order; LEVELS levels hold up to 2^LEVELS - 1 items ... and 2^(LEVELS-1)
// exactly fills the top
template <int LEVELS> struct FwCounterRef {
    double lvl[LEVELS];
    long long n = 0;
    void push(double v) {
        const long long j = n++;
        for (int k = 0; k < LEVELS; ++k) {
            if ((j >> k) & 1) {
                v = fw_add(lvl[k], v);
            } else {
                lvl[k] = v;
                return;
            }
        }
    }
    double close() const { // the occupied levels from the lowest up: the missing ones are padding
        double acc = 0.0;
        bool have = false;
        for (int k = 0; k < LEVELS; ++k)
            if ((n >> k) & 1) {
                acc = have ? fw_add(lvl[k], acc) : lvl[k];
                have = true;
            }
        return acc;
    }
};
// entries [lo, hi) of a row (hi - lo <= piece): rounds of FW_SLOTS by the butterfly, the rounds through the counter
inline double fw_piece_sum_ref(const double *t, long long lo, long long hi) {
    FwCounterRef<FW_LEVELS_LONG> c;
    for (long long e0 = lo; e0 < hi; e0 += FW_SLOTS) {
        double s[FW_SLOTS];
        for (int j = 0; j < FW_SLOTS; ++j) s[j] = e0 + j < hi ? t[e0 + j] : 0.0;
        for (int len = FW_SLOTS; len > 1; len /= 2)
            for (int j = 0; j < len / 2; ++j) s[j] = fw_add(s[2 * j], s[2 * j + 1]);
        c.push(s[0]);
    }
    return c.close();
}
inline double fw_row_sum_ref(const double *t, long long len, int piece) {
    if (len <= 0) return 0.0;
    if (!fw_row_long(len, piece)) return fw_piece_sum_ref(t, 0, len);
    const long long np = fw_pieces(len, piece), pb = fw_block_pieces(piece);
    double acc = 0.0;
    for (long long b = 0; b * pb < np; ++b) {
        FwCounterRef<FW_BLOCK_LEVELS> c;
        for (long long k = b * pb; k < np && k < (b + 1) * pb; ++k) c.push(fw_piece_sum_ref(t, fw_piece_lo(piece, k), fw_piece_hi(len, piece, k)));
        acc = b == 0 ? c.close() : fw_add(acc, c.close());
    }
    return acc;
}

} // namespace dppr
