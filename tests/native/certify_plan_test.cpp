// certify_plan_test.cpp -- dynamicppr_amd/csrc/dppr_certify_plan.hpp on the CPU: every rejection of a call's arguments at its
// limit, the hook's values, which outputs a call computes, the layout of the result block for every combination of NULL and
// non-NULL outputs -- planes that do not overlap, 8-byte planes at multiples of 8, room only for what is asked --, the pieces of
// a row (every edge covered exactly once) with the bound of their list, the shape of the gather and the work space.
// Every array is exactly as long as the code may touch (the sanitizers watch the bounds).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_certify_plan.hpp"

using namespace dppr;

static int failures = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            ++failures;                      \
            std::printf("FAIL %s: ", #cond); \
            std::printf(__VA_ARGS__);        \
            std::printf("\n");               \
        }                                    \
    } while (0)

static void arguments() {
    dppr_certify_out_t out{};
    const double tiny = std::numeric_limits<double>::denorm_min(), inf = std::numeric_limits<double>::infinity();
    CHECK(cert_args_ok(1e-9, DPPR_CERT_RESIDUAL | DPPR_CERT_INVARIANT, &out), "a plain call");
    CHECK(cert_args_ok(1e-9, DPPR_CERT_RESIDUAL, &out) && cert_args_ok(1e-9, DPPR_CERT_INVARIANT, &out), "either part alone");
    CHECK(!cert_args_ok(1e-9, 3, nullptr), "a NULL out");
    CHECK(!cert_args_ok(1e-9, 0, &out) && !cert_args_ok(1e-9, 4, &out) && !cert_args_ok(1e-9, -1, &out), "flags outside 1 .. 3");
    CHECK(cert_args_ok(tiny, 3, &out) && cert_args_ok(inf, 3, &out), "the smallest positive eps, and +inf");
    CHECK(!cert_args_ok(0.0, 3, &out) && !cert_args_ok(-0.0, 3, &out) && !cert_args_ok(-1e-9, 3, &out), "an eps that is not positive");
    CHECK(!cert_args_ok(std::nan(""), 3, &out), "a NaN eps");

    CHECK(cert_hook_ok(0, 0) && cert_hook_ok(7, 1) && cert_hook_ok(64, 4) && cert_hook_ok(CERT_PIECE_MAX, 64), "the hook's values");
    CHECK(!cert_hook_ok(-1, 0) && !cert_hook_ok(CERT_PIECE_MAX + 1, 0) && !cert_hook_ok(0, -1) && !cert_hook_ok(0, 3) && !cert_hook_ok(0, 128),
          "the hook's rejections");
    CHECK(cert_piece(0) == CERT_PIECE && cert_piece(7) == 7, "0 leaves the piece to the plan");
}

static void which_bits() {
    double d = 0;
    int32_t i = 0;
    int64_t l = 0;
    dppr_certify_out_t out{};
    CHECK(cert_which(nullptr, 3) == 0 && cert_which(&out, 3) == 0, "nothing asked");
    out.max_abs_r = &d, out.argmax_r = &i, out.sum_abs_r = &d, out.sum_p = &d;
    out.n_pos = &l, out.n_neg = &l, out.n_nonfinite = &l, out.n_p_nonzero = &l;
    out.inv_max_err = &d, out.inv_argmax = &i;
    CHECK(cert_which(&out, 3) == (CERT_RES | CERT_INV), "everything");
    CHECK(cert_which(&out, DPPR_CERT_RESIDUAL) == CERT_RES && cert_which(&out, DPPR_CERT_INVARIANT) == CERT_INV, "a part the flags leave out is not run");
    out.inv_max_err = nullptr, out.inv_argmax = nullptr;
    CHECK(cert_which(&out, DPPR_CERT_INVARIANT) == 0, "INVARIANT with every invariant pointer NULL: nothing to run");
    CHECK(cert_which(&out, 3) == CERT_RES, "... and the residual part alone beside it");
    dppr_certify_out_t one{};
    one.n_nonfinite = &l;
    CHECK(cert_which(&one, 3) == CERT_N_NONFINITE, "one pointer, one bit");
}

static void layout() {
    struct Plane {
        uint32_t bit;
        size_t CertLayout::*off;
        size_t elem;
    };
    const Plane planes[] = {{CERT_MAX_R, &CertLayout::off_max_r, 8},           {CERT_SUM_R, &CertLayout::off_sum_r, 8},
                            {CERT_SUM_P, &CertLayout::off_sum_p, 8},           {CERT_INV_ERR, &CertLayout::off_inv_err, 8},
                            {CERT_N_POS, &CertLayout::off_n_pos, 8},           {CERT_N_NEG, &CertLayout::off_n_neg, 8},
                            {CERT_N_NONFINITE, &CertLayout::off_n_nonfinite, 8}, {CERT_N_P_NONZERO, &CertLayout::off_n_p_nonzero, 8},
                            {CERT_ARGMAX_R, &CertLayout::off_argmax_r, 4},     {CERT_INV_ARG, &CertLayout::off_inv_arg, 4}};
    for (int n : {1, 2, 5, 15, 16})
        for (uint32_t which = 0; which < (1u << 10); ++which) {
            const CertLayout l = cert_layout(n, which);
            std::vector<unsigned char> used(l.total_bytes, 0); // (the sanitizers watch every plane's end)
            size_t asked = 0;
            bool ok = true;
            for (const Plane &p : planes) {
                if (!(which & p.bit)) continue;
                const size_t off = l.*(p.off), bytes = p.elem * (size_t)n;
                if (p.elem == 8 && off % 8) ok = false;
                if (off % 4) ok = false;
                for (size_t b = off; b < off + bytes; ++b) {
                    if (used[b]) ok = false;
                    used[b] = 1;
                }
                asked += bytes;
            }
            CHECK(ok, "n %d which 0x%x: a plane overlaps another or is misaligned", n, which);
            CHECK(l.copy_bytes == asked, "n %d which 0x%x: room only for what is asked (%zu != %zu)", n, which, l.copy_bytes, asked);
            CHECK(l.total_bytes >= l.copy_bytes && l.total_bytes >= 8 && l.total_bytes % 8 == 0 && l.total_bytes < l.copy_bytes + 16,
                  "n %d which 0x%x: the block is the copy, padded", n, which);
        }
}

static void pieces() {
    for (int piece : {1, 7, 64, CERT_PIECE}) {
        for (long long len : {0ll, 1ll, (long long)piece - 1, (long long)piece, (long long)piece + 1, 3ll * piece, 3ll * piece + 1}) {
            if (len < 0) continue;
            const long long np = cert_row_pieces(len, piece);
            std::vector<int> seen((size_t)len, 0);
            bool ok = true;
            for (long long k = 0; k < np; ++k) {
                const long long lo = cert_piece_lo(piece, k), hi = cert_piece_hi(len, piece, k);
                if (!(lo < hi && hi - lo <= piece && hi <= len)) ok = false;
                if (k + 1 < np && hi - lo != piece) ok = false; // (only the last piece is short)
                for (long long e = lo; e < hi && e < len; ++e) ++seen[(size_t)e];
            }
            CHECK(ok, "piece %d len %lld: a piece is empty, too long or leaves the row", piece, len);
            CHECK(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }), "piece %d len %lld: every edge exactly once", piece, len);
            CHECK(np == (len + piece - 1) / piece, "piece %d len %lld: %lld pieces", piece, len, np);
            CHECK(cert_row_long(len, piece) == (np >= 2), "piece %d len %lld: a row is long iff it has two pieces or more", piece, len);
        }
    }
    CHECK(cert_row_pieces(0, 7) == 0 && cert_row_pieces(1, 7) == 1 && cert_row_pieces(6, 7) == 1 && cert_row_pieces(7, 7) == 1 &&
              cert_row_pieces(8, 7) == 2 && cert_row_pieces(21, 7) == 3,
          "the piece counts of the stated lengths");
    // the bound of the list: the worst graphs -- as many rows of piece + 1 edges as Ed holds (two pieces each), one row of Ed edges
    for (int piece : {1, 7, 64, CERT_PIECE})
        for (long long Ed : {0ll, 1ll, (long long)piece, (long long)piece + 1, 1000ll, 1000003ll, 2147483647ll}) {
            const size_t cap = cert_list_cap(Ed, piece);
            const long long rows = Ed / (piece + 1), rest = Ed - rows * (piece + 1);
            const long long many = rows * cert_row_pieces(piece + 1, piece) + (cert_row_long(rest, piece) ? cert_row_pieces(rest, piece) : 0);
            const long long one = cert_row_long(Ed, piece) ? cert_row_pieces(Ed, piece) : 0;
            CHECK((size_t)many <= cap && (size_t)one <= cap, "piece %d Ed %lld: %lld / %lld queued pieces above the cap %zu", piece, Ed, many, one, cap);
        }
    CHECK(cert_item_row(cert_item(0xfffffffeu, 5)) == 0xfffffffeu && cert_item_piece(cert_item(3, 0xffffffffu)) == 0xffffffffu, "an item keeps both halves");
}

static void shape() {
    for (int gw : {1, 2, 4, 6, 8, 10, 12, 14, 16}) {
        const int T = cert_team(gw);
        CHECK((T & (T - 1)) == 0 && T >= 1 && T <= 8 && (gw == 1 ? T == 1 : 2 * T >= gw) && (T == 1 || T < gw), "gw %d: a team of %d lanes covers the row in 16-byte pieces", gw, T);
        for (int forced : {0, 1, 2, 4, 8, 16, 32, 64}) {
            const int wr = cert_wave_rows(gw, forced);
            CHECK(wr >= 1 && (wr & (wr - 1)) == 0 && 64 / wr >= T && (64 / wr) % T == 0, "gw %d forced %d: every row's segment holds whole teams", gw, forced);
            CHECK(forced == 0 || wr == std::min(forced, 64 / T), "gw %d forced %d: the hook's number, capped by the teams of a wave", gw, forced);
        }
    }
    for (int n = 1; n <= 16; ++n) {
        const int lw = cert_lane_stride(n);
        CHECK(lw >= n && lw < 2 * n && (lw & (lw - 1)) == 0 && CERT_BLOCK % lw == 0, "n %d: the lanes rounded up to a power of two", n);
    }
    CHECK(cert_stream_grid(0) == 1 && cert_stream_grid(1) == 1 && cert_stream_grid(2049) == 2 && cert_stream_grid(1ll << 31) == CERT_GRID_MAX,
          "one workgroup per tile, CERT_GRID_MAX at the most");
    CHECK(cert_rows_grid(0, 4) == 1 && cert_rows_grid(16, 4) == 1 && cert_rows_grid(17, 4) == 2 && cert_rows_grid(1ll << 31, 1) == 8 * CERT_GRID_MAX, "the grid of the gather");
    const CertWork w = cert_work();
    CHECK(w.off_head == 0 && w.off_sums >= sizeof(CertHead) && w.off_sums % 8 == 0 && w.off_max_r == w.off_sums + 8 * 2 * Q_LANES &&
              w.off_max_inv == w.off_max_r + sizeof(CertMax) * CERT_GRID_MAX * Q_LANES && w.bytes == w.off_max_inv + sizeof(CertMax) * CERT_GRID_MAX * Q_LANES,
          "the work space: head, sums, one partial per workgroup and lane of either pass");
    CHECK(sizeof(CertMax) == 16, "a partial is a word and an id");
    CHECK(cert_part_elems(0, 3) == (size_t)2 * 3 * DOT_TPB && cert_part_elems(70000, 16) == (size_t)2 * 16 * 2 * DOT_TPB, "the partials of the two sums: whole blocks");
}

int main() {
    arguments();
    which_bits();
    layout();
    pieces();
    shape();
    std::printf("certify_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
