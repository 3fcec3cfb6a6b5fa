// dppr_certify_plan.hpp -- what the certificate of a state (dppr_certify / dppr_group_certify) decides before any device is
// involved: the rejections, which outputs a call asks for, the layout of the result block (only the planes asked for have room,
// the 8-byte planes first), the pieces a long out-row is cut into with the bound of their list, the grids, and what
// dppr_debug_certify changes. Pure host code without HIP includes (dppr_host_query.hpp checks a call and lays it out with it,
// dppr_certify.hpp takes its constants and its piece arithmetic; tests/native/certify_plan_test.cpp drives it on the CPU under the
// sanitizers).
//
// BLOCK, one copy to the host, every plane [n]:
//   max_abs_r | sum_abs_r | sum_p | inv_max_err | n_pos | n_neg | n_nonfinite | n_p_nonzero        (8-byte elements)
//   argmax_r | inv_argmax                                                                          (int32)
// PIECES. An out-row of len stored edges is walked in cert_row_pieces(len, piece) pieces of at most `piece` edges, piece k the
// edges [k * piece, min(len, (k + 1) * piece)) of the row. A row of one piece is summed where it is met; a row of two or more is
// LONG: its pieces are queued, every piece writes one [gw] partial, and the row's sum is its partials added in piece order.
#pragma once

#include "dppr_dot_plan.hpp"
#include "dppr_query_plan.hpp"

namespace dppr {

constexpr int CERT_BLOCK = 256;            // every kernel of dppr_certify.hpp: four waves
constexpr int CERT_WAVES = CERT_BLOCK / 64;
constexpr int CERT_PIECE = 2048;           // edges of a piece (dppr_debug_certify lowers it)
constexpr int CERT_PIECE_MAX = 1 << 20;
constexpr int CERT_WAVE_ROWS = 4;          // short rows that share a wave of the gather (dppr_debug_certify changes it)
constexpr int CERT_GRID_MAX = 2048;        // workgroups of a streaming pass at the most: one max / arg-max partial each

enum : uint32_t { // the outputs of a call, one bit per pointer of dppr_certify_out_t
    CERT_MAX_R = 1u << 0, CERT_ARGMAX_R = 1u << 1, CERT_SUM_R = 1u << 2, CERT_SUM_P = 1u << 3, CERT_N_POS = 1u << 4,
    CERT_N_NEG = 1u << 5, CERT_N_NONFINITE = 1u << 6, CERT_N_P_NONZERO = 1u << 7, CERT_INV_ERR = 1u << 8, CERT_INV_ARG = 1u << 9,
    CERT_RES = CERT_MAX_R | CERT_ARGMAX_R | CERT_SUM_R | CERT_SUM_P | CERT_N_POS | CERT_N_NEG | CERT_N_NONFINITE | CERT_N_P_NONZERO,
    CERT_INV = CERT_INV_ERR | CERT_INV_ARG,
};

// eps > 0 is false for a NaN
inline bool cert_args_ok(double eps, int flags, const dppr_certify_out_t *out) {
    return out && flags >= 1 && flags <= (DPPR_CERT_RESIDUAL | DPPR_CERT_INVARIANT) && eps > 0.0;
}
// dppr_debug_certify: 0 leaves a choice to the plan; wave_rows a power of two
inline bool cert_hook_ok(int piece_edges, int wave_rows) {
    return piece_edges >= 0 && piece_edges <= CERT_PIECE_MAX && wave_rows >= 0 && wave_rows <= 64 && (wave_rows & (wave_rows - 1)) == 0;
}
constexpr int cert_piece(int forced) { return forced > 0 ? forced : CERT_PIECE; }

// what a call computes: the pointers that are not NULL, of the parts `flags` names
inline uint32_t cert_which(const dppr_certify_out_t *o, int flags) {
    if (!o) return 0;
    uint32_t w = 0;
    if (flags & DPPR_CERT_RESIDUAL) {
        if (o->max_abs_r) w |= CERT_MAX_R;
        if (o->argmax_r) w |= CERT_ARGMAX_R;
        if (o->sum_abs_r) w |= CERT_SUM_R;
        if (o->sum_p) w |= CERT_SUM_P;
        if (o->n_pos) w |= CERT_N_POS;
        if (o->n_neg) w |= CERT_N_NEG;
        if (o->n_nonfinite) w |= CERT_N_NONFINITE;
        if (o->n_p_nonzero) w |= CERT_N_P_NONZERO;
    }
    if (flags & DPPR_CERT_INVARIANT) {
        if (o->inv_max_err) w |= CERT_INV_ERR;
        if (o->inv_argmax) w |= CERT_INV_ARG;
    }
    return w;
}

struct CertLayout {
    size_t off_max_r = 0, off_sum_r = 0, off_sum_p = 0, off_inv_err = 0;
    size_t off_n_pos = 0, off_n_neg = 0, off_n_nonfinite = 0, off_n_p_nonzero = 0;
    size_t off_argmax_r = 0, off_inv_arg = 0;
    size_t copy_bytes = 0, total_bytes = 0;
};
constexpr CertLayout cert_layout(int n, uint32_t which) {
    CertLayout l;
    size_t at = 0;
    auto take = [&](uint32_t bit, size_t elem_bytes) {
        const size_t here = at;
        if (which & bit) at += (size_t)n * elem_bytes;
        return here;
    };
    l.off_max_r = take(CERT_MAX_R, sizeof(double));
    l.off_sum_r = take(CERT_SUM_R, sizeof(double));
    l.off_sum_p = take(CERT_SUM_P, sizeof(double));
    l.off_inv_err = take(CERT_INV_ERR, sizeof(double));
    l.off_n_pos = take(CERT_N_POS, sizeof(int64_t));
    l.off_n_neg = take(CERT_N_NEG, sizeof(int64_t));
    l.off_n_nonfinite = take(CERT_N_NONFINITE, sizeof(int64_t));
    l.off_n_p_nonzero = take(CERT_N_P_NONZERO, sizeof(int64_t));
    l.off_argmax_r = take(CERT_ARGMAX_R, sizeof(int32_t));
    l.off_inv_arg = take(CERT_INV_ARG, sizeof(int32_t));
    l.copy_bytes = at;
    l.total_bytes = pad8(at);
    if (l.total_bytes < 8) l.total_bytes = 8; // (a buffer of no bytes is not one)
    return l;
}

// ---- the pieces of an out-row --------------------------------------------------------------------------------------------
constexpr long long cert_row_pieces(long long len, int piece) { return len <= 0 ? 0 : (len + piece - 1) / piece; }
constexpr long long cert_piece_lo(int piece, long long k) { return k * piece; }
constexpr long long cert_piece_hi(long long len, int piece, long long k) { return (k + 1) * piece < len ? (k + 1) * piece : len; }
constexpr bool cert_row_long(long long len, int piece) { return len > piece; }
// Pieces the long rows of a graph of Ed edges can queue: a long row has len > piece, so its ceil(len / piece) pieces are fewer
// than len / piece + 1 < 2 len / piece, and the long rows together hold at most Ed edges.
constexpr size_t cert_list_cap(long long Ed, int piece) { return (size_t)(2 * (Ed / piece) + 2); }
// a queued piece: row (internal id) << 32 | piece number
constexpr unsigned long long cert_item(unsigned row, unsigned k) { return ((unsigned long long)row << 32) | k; }
constexpr unsigned cert_item_row(unsigned long long it) { return (unsigned)(it >> 32); }
constexpr unsigned cert_item_piece(unsigned long long it) { return (unsigned)it; }

// ---- the shape of the gather ---------------------------------------------------------------------------------------------
// lanes of a team: one per 16 bytes of a row of gw doubles (a slot's row of one double: one lane), rounded up to a power of two
constexpr int cert_team(int gw) { return gw <= 2 ? 1 : gw <= 4 ? 2 : gw <= 8 ? 4 : 8; }
// short rows that share a wave: the hook's or the plan's number, never more than the wave has teams
constexpr int cert_wave_rows(int gw, int forced) {
    const int teams = 64 / cert_team(gw);
    const int want = forced > 0 ? forced : CERT_WAVE_ROWS;
    return want < teams ? want : teams;
}
// threads that share a row of the streaming passes: the lanes rounded up to a power of two
constexpr int cert_lane_stride(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16; }

constexpr int cert_stream_grid(int64_t V) {
    const int64_t tiles = dot_tiles(V);
    return tiles < 1 ? 1 : tiles < CERT_GRID_MAX ? (int)tiles : CERT_GRID_MAX;
}
constexpr int cert_rows_grid(int64_t live_rows, int wave_rows) {
    const int64_t per_wg = (int64_t)CERT_WAVES * wave_rows;
    const int64_t g = (live_rows + per_wg - 1) / per_wg;
    return g < 1 ? 1 : g < 8 * CERT_GRID_MAX ? (int)g : 8 * CERT_GRID_MAX;
}

// ---- the work space on the device ------------------------------------------------------------------------------------------
// the head (zeroed per call): the four counters of every lane, the number of queued pieces; then what the passes leave for
// k_cert_finish: the two sums [2][16], and one (word, id) partial per workgroup and lane of either streaming pass
struct CertHead {
    unsigned long long n_pos[Q_LANES], n_neg[Q_LANES], n_nonfinite[Q_LANES], n_p_nonzero[Q_LANES];
    unsigned n_items, pad;
    DotHead dot; // (never raised: k_dot_combine reads it)
};
struct CertMax { // the largest word a workgroup met and the smallest external id that attains it (0x7fffffff: none)
    unsigned long long word;
    int id, pad;
};
struct CertWork {
    size_t off_head = 0, off_sums = 0, off_max_r = 0, off_max_inv = 0, bytes = 0;
};
constexpr CertWork cert_work() {
    CertWork w;
    w.off_sums = pad8(sizeof(CertHead));
    w.off_max_r = w.off_sums + sizeof(double) * 2 * Q_LANES;
    w.off_max_inv = w.off_max_r + sizeof(CertMax) * (size_t)CERT_GRID_MAX * Q_LANES;
    w.bytes = w.off_max_inv + sizeof(CertMax) * (size_t)CERT_GRID_MAX * Q_LANES;
    return w;
}
// doubles of the dot family's partials the two sums take: [2 n outputs][whole blocks of tiles]
constexpr size_t cert_part_elems(int64_t V, int n) { return (size_t)2 * (size_t)n * (size_t)(dot_cols(V) > 0 ? dot_cols(V) : DOT_TPB); }

} // namespace dppr
