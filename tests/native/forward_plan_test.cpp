// forward_plan_test.cpp -- dynamicppr_amd/csrc/dppr_forward_plan.hpp on the CPU: every rejection of a call's arguments at its
// limit, which parts a call asks for and when a part is complete, the hook's values, the check schedule against its plain
// statement, the team / segment shapes of every row width, the pieces of a row (every entry covered exactly once, aligned) with
// the bounds of their lists, and the row sum as the device forms it -- rounds of 8 by neighbours, a counter over the rounds, a
// counter over the pieces of a block, the blocks in order -- against the fold of the contract (dot_fold_ref) bit for bit.
// Every array is exactly as long as the code may touch (the sanitizers watch the bounds).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_forward_plan.hpp"

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
    dppr_forward_out_t out{};
    const int32_t s[1] = {0};
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(fw_args_ok(s, 1, 1, 0.0, &out) && fw_args_ok(s, 16, 256, 1e-3, &out), "the limits are inside");
    CHECK(!fw_args_ok(s, 0, 8, 0.0, &out) && !fw_args_ok(s, 17, 8, 0.0, &out) && !fw_args_ok(s, -1, 8, 0.0, &out), "m outside 1 .. 16");
    CHECK(!fw_args_ok(s, 1, 0, 0.0, &out) && !fw_args_ok(s, 1, 257, 0.0, &out) && !fw_args_ok(s, 1, -8, 0.0, &out), "iters outside 1 .. 256");
    CHECK(!fw_args_ok(s, 1, 8, -1e-300, &out) && !fw_args_ok(s, 1, 8, std::nan(""), &out) && !fw_args_ok(s, 1, 8, inf, &out) &&
              !fw_args_ok(s, 1, 8, -inf, &out),
          "a tol that is negative or not finite");
    CHECK(fw_args_ok(s, 1, 8, -0.0, &out) && fw_args_ok(s, 1, 8, std::numeric_limits<double>::max(), &out), "-0.0 is 0; the largest finite tol");
    CHECK(!fw_args_ok(nullptr, 1, 8, 0.0, &out) && !fw_args_ok(s, 1, 8, 0.0, nullptr), "a NULL starts, a NULL out");

    CHECK(fw_hook_ok(0, 0) && fw_hook_ok(64, 1) && fw_hook_ok(4096, 8) && fw_hook_ok(512, 2) && fw_hook_ok(0, 4), "the hook's values");
    CHECK(!fw_hook_ok(32, 0) && !fw_hook_ok(8192, 0) && !fw_hook_ok(96, 0) && !fw_hook_ok(-64, 0) && !fw_hook_ok(0, 3) && !fw_hook_ok(0, 16) &&
              !fw_hook_ok(0, -1),
          "the hook's rejections");
    CHECK(fw_piece(0) == FW_PIECE && fw_piece(64) == 64 && fw_levels(64) == FW_LEVELS_SHORT && fw_levels(FW_PIECE) == FW_LEVELS_SHORT &&
              fw_levels(1024) == FW_LEVELS_LONG && fw_levels(4096) == FW_LEVELS_LONG,
          "0 leaves the piece to the plan; the counter a piece needs");
}

static void parts() {
    dppr_forward_out_t o{};
    int32_t i = 0;
    double d = 0;
    CHECK(fw_which(nullptr) == 0 && fw_which(&o) == 0 && fw_parts_ok(&o), "nothing asked: nothing to complete");
    o.rem = &d;
    CHECK(fw_which(&o) == FW_META, "rem alone");
    o.rem = nullptr, o.iters_used = &i;
    CHECK(fw_which(&o) == FW_META && fw_parts_ok(&o), "iters_used alone");
    o.topk_f = &d;
    CHECK(fw_which(&o) == (FW_META | FW_TOPK) && !fw_parts_ok(&o), "a top-k part with pointers missing");
    o.topk_ids = &i, o.topk_counts = &i, o.k = 0;
    CHECK(!fw_parts_ok(&o), "k = 0");
    o.k = DPPR_TOPK_MAX + 1;
    CHECK(!fw_parts_ok(&o), "k beyond DPPR_TOPK_MAX");
    o.k = DPPR_TOPK_MAX, o.min_f = -1e-9;
    CHECK(!fw_parts_ok(&o), "a negative min_f");
    o.min_f = std::nan("");
    CHECK(!fw_parts_ok(&o), "a NaN min_f");
    o.min_f = 0.0;
    CHECK(fw_parts_ok(&o), "the complete top-k part");
    o.at_f = &d;
    CHECK((fw_which(&o) & FW_AT) && !fw_parts_ok(&o), "at_f without at_ids");
    o.at_ids = &i, o.n_at = 0;
    CHECK(!fw_parts_ok(&o), "n_at = 0");
    o.n_at = DPPR_FORWARD_AT_MAX + 1;
    CHECK(!fw_parts_ok(&o), "n_at beyond the limit");
    o.n_at = DPPR_FORWARD_AT_MAX;
    CHECK(fw_parts_ok(&o), "the complete at part");
    o.dense_dev = &d, o.dense_dtype = 2;
    CHECK((fw_which(&o) & FW_DENSE) && !fw_parts_ok(&o), "a dtype that is none");
    o.dense_dtype = DPPR_F32, o.dense_layout = 2;
    CHECK(!fw_parts_ok(&o), "a layout that is none");
    o.dense_layout = DPPR_SOURCE_MAJOR;
    CHECK(fw_parts_ok(&o) && fw_which(&o) == (FW_META | FW_TOPK | FW_AT | FW_DENSE), "every part");
}

static void schedule() {
    for (int iters = 1; iters <= DPPR_FORWARD_MAX_ITERS; ++iters) {
        std::vector<int> want;
        for (int k = 8; k < iters; k += 8) want.push_back(k);
        want.push_back(iters);
        std::vector<int> got, chunks;
        for (int k = 1; k <= iters; ++k)
            if (fw_is_check(k, iters)) got.push_back(k);
        for (int k = 0; k < iters;) chunks.push_back(k = fw_next_check(k, iters));
        CHECK(got == want && chunks == want, "the checks of iters = %d", iters);
        CHECK(fw_rowless_iters(iters) == want[0], "a start without a row stops at the first check (iters = %d)", iters);
    }
}

static void shapes() {
    for (int m = 1; m <= 16; ++m) {
        const int gw = fw_row_width(m);
        CHECK(gw >= m && gw % 2 == 0 && gw <= 16 && gw - m <= (m == 1 ? 1 : 1), "the row width of m = %d", m);
        for (int forced : {0, 1, 2, 4, 8}) {
            const int T = fw_team(gw, forced), pp = fw_lane_pieces(gw, T);
            CHECK((T & (T - 1)) == 0 && T >= 1 && T <= 8 && (forced == 0 || T >= forced), "a team of m = %d, forced %d: %d", m, forced, T);
            CHECK(pp >= 1 && pp <= 2 && pp * T >= fw_row_pieces(gw), "the team covers the row with at most two pieces a lane (m = %d, T = %d)", m, T);
            CHECK(fw_segment(T) * fw_wave_rows(T) == 64 && fw_wave_rows(T) >= 1, "the segments fill the wave (T = %d)", T);
            if (forced == 0) CHECK(pp == 1, "the plan's team takes one piece a lane (m = %d)", m);
            CHECK(fw_units_grid(0, T) == 1 && fw_units_grid(1 << 30, T) == FW_GRID_MAX, "the grid of T = %d is bounded", T);
        }
    }
    CHECK(fw_team(16, 1) == 4 && fw_team(16, 0) == 8 && fw_team(2, 0) == 1 && fw_team(2, 8) == 8 && fw_team(10, 2) == 4 && fw_team(6, 1) == 2,
          "teams by hand");
    CHECK(fw_all(1) == 1u && fw_all(16) == 0xffffu, "the word of all columns");
    CHECK(fw_plane_elems(0, 2) == 2 && fw_plane_elems(1000, 16) == 16000 && fw_part_elems(1, 3) == 3 * (size_t)DOT_TPB &&
              fw_part_elems(70000, 2) == 2 * 2 * (size_t)DOT_TPB,
          "the planes and the partials");
}

static void pieces() {
    for (int piece : {64, 512, 4096}) {
        CHECK(fw_block_pieces(piece) * (long long)piece == DOT_BLOCK, "pieces tile a block (piece = %d)", piece);
        for (long long len : {0ll, 1ll, (long long)piece - 1, (long long)piece, (long long)piece + 1, 3ll * piece, 65536ll, 65537ll, 200000ll}) {
            const long long np = fw_pieces(len, piece);
            std::vector<int> seen((size_t)len, 0);
            for (long long k = 0; k < np; ++k) {
                const long long lo = fw_piece_lo(piece, k), hi = fw_piece_hi(len, piece, k);
                CHECK(lo % piece == 0 && lo < hi && hi - lo <= piece && hi <= len, "piece %lld of a row of %lld", k, len);
                for (long long e = lo; e < hi; ++e) seen[(size_t)e]++;
            }
            bool once = true;
            for (int c : seen) once = once && c == 1;
            CHECK(once, "every entry of a row of %lld in exactly one piece of %d", len, piece);
            CHECK(fw_row_long(len, piece) == (np >= 2), "long means two pieces or more (len = %lld)", len);
        }
        // the bounds of the lists on graphs made of long rows alone, the worst case: rows of piece + 1 entries
        for (long long rows : {1ll, 7ll, 1000ll}) {
            const long long Ed = rows * (piece + 1);
            CHECK((size_t)(rows * fw_pieces(piece + 1, piece)) <= fw_item_cap(Ed, piece) && (size_t)rows <= fw_long_cap(Ed, piece),
                  "the lists hold %lld rows of piece + 1", rows);
        }
        CHECK(fw_item_cap(0, piece) >= 1 && fw_long_cap(0, piece) >= 1, "an empty graph still has a list");
    }
    CHECK(fw_item_row(fw_item(0xfffffffeu, 12345u)) == 0xfffffffeu && fw_item_piece(fw_item(7u, 0xffffffffu)) == 0xffffffffu, "an item keeps both words");
}

// the device's row sum is the fold of the contract, for every piece size, bit for bit
static void row_sums() {
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return (double)(s >> 11) / 9007199254740992.0; // [0, 1): every term >= +0.0
    };
    for (long long len : {0ll, 1ll, 2ll, 7ll, 8ll, 9ll, 63ll, 64ll, 65ll, 511ll, 512ll, 513ll, 4095ll, 4096ll, 4097ll, 65535ll, 65536ll, 65537ll,
                          70001ll, 131073ll}) {
        std::vector<double> t((size_t)len);
        for (auto &v : t) v = rnd() * std::ldexp(1.0, -(int)(s % 40)); // many magnitudes: the order of the additions shows
        if (len > 3) t[(size_t)len / 2] = 0.0;
        const double want = dot_fold_ref(t.data(), len);
        double plain = 0.0;
        for (double v : t) plain = fw_add(plain, v);
        for (int piece : {64, 128, 512, 1024, 4096}) {
            const double got = fw_row_sum_ref(t.data(), len, piece);
            CHECK(std::memcmp(&got, &want, 8) == 0, "len %lld piece %d: %.17g against the fold's %.17g", len, piece, got, want);
        }
        if (len == 70001) CHECK(plain != want, "the running sum is another number: the comparison can fail");
    }
    // the counter alone: 2^k items fill level k, and a count that is no power of two closes as the padded tree
    FwCounterRef<4> c;
    for (int i = 1; i <= 5; ++i) c.push((double)i);
    CHECK(c.close() == ((1.0 + 2.0) + (3.0 + 4.0)) + 5.0, "five items: the tree over eight slots");
}

int main() {
    arguments();
    parts();
    schedule();
    shapes();
    pieces();
    row_sums();
    std::printf("forward_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
