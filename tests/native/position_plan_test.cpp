// position_plan_test.cpp -- dynamicppr_amd/csrc/dppr_position_plan.hpp on the CPU: every rejection of a call's arguments at its
// limit, the shape of the count pass for every (n, m, tile) -- its LDS never above the 160 KiB of a CU, two workgroups of it
// inside them, and its lane blocks, passes and slots covering every (lane, position) pair exactly once against a brute-force walk
// of the grid --, the grid's first dimension, the layout of the workspace and of the result block.
// Every array is exactly as long as the code may touch (the sanitizers watch the bounds).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_position_plan.hpp"

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
    const int64_t V = 100;
    std::vector<int32_t> ids(DPPR_POSITION_MAX, 7), over(DPPR_POSITION_MAX + 1, 7), pos(4);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(position_args_ok(nullptr, 0.0, ids.data(), 4, V, pos.data()), "a plain call");
    CHECK(position_args_ok(nullptr, 0.0, ids.data(), DPPR_POSITION_MAX, V, pos.data()), "m at the limit");
    CHECK(!position_args_ok(nullptr, 0.0, over.data(), DPPR_POSITION_MAX + 1, V, pos.data()), "m above the limit");
    CHECK(!position_args_ok(nullptr, 0.0, ids.data(), -1, V, pos.data()), "m < 0");
    CHECK(position_args_ok(nullptr, 0.0, nullptr, 0, V, nullptr), "m == 0 needs neither ids nor pos");
    CHECK(!position_args_ok(nullptr, 0.0, nullptr, 1, V, pos.data()), "NULL ids with m > 0");
    CHECK(!position_args_ok(nullptr, 0.0, ids.data(), 1, V, nullptr), "NULL pos with m > 0");
    CHECK(position_args_ok(nullptr, inf, ids.data(), 1, V, pos.data()) && position_args_ok(nullptr, 1e-300, ids.data(), 1, V, pos.data()), "min_score >= 0");
    CHECK(position_args_ok(nullptr, -0.0, ids.data(), 1, V, pos.data()), "-0.0 is 0");
    CHECK(!position_args_ok(nullptr, -1e-300, ids.data(), 1, V, pos.data()) && !position_args_ok(nullptr, nan, ids.data(), 1, V, pos.data()) &&
              !position_args_ok(nullptr, -inf, ids.data(), 1, V, pos.data()),
          "min_score negative or NaN");
    std::vector<int32_t> edge = {0, (int32_t)V - 1};
    CHECK(position_args_ok(nullptr, 0.0, edge.data(), 2, V, pos.data()), "ids at both ends of [0, V)");
    edge[1] = (int32_t)V;
    CHECK(!position_args_ok(nullptr, 0.0, edge.data(), 2, V, pos.data()), "an id == V");
    edge[1] = -1;
    CHECK(!position_args_ok(nullptr, 0.0, edge.data(), 2, V, pos.data()), "an id < 0");
    CHECK(position_args_ok(nullptr, 0.0, edge.data(), 1, V, pos.data()), "only m ids are read");
    dppr_rank_spec_t s{};
    CHECK(position_args_ok(&s, 0.0, ids.data(), 1, V, pos.data()), "the zero spec");
    s.factor = 4;
    CHECK(!position_args_ok(&s, 0.0, ids.data(), 1, V, pos.data()) && !position_args_ok(&s, 0.0, nullptr, 0, V, nullptr), "an unknown factor, also at m == 0");
    s.factor = DPPR_FACTOR_DEV;
    s.factor_dtype = 2;
    CHECK(!position_args_ok(&s, 0.0, ids.data(), 1, V, pos.data()), "an unknown dtype");
    s = dppr_rank_spec_t{};
    s.mask = 3;
    CHECK(!position_args_ok(&s, 0.0, ids.data(), 1, V, pos.data()), "an unknown mask");
    s = dppr_rank_spec_t{};
    s.exclude = 8;
    CHECK(!position_args_ok(&s, 0.0, ids.data(), 1, V, pos.data()), "an unknown exclude bit");
    CHECK(position_tile_ok(0) && position_tile_ok(1) && position_tile_ok(DPPR_POSITION_MAX) && !position_tile_ok(-1) && !position_tile_ok(DPPR_POSITION_MAX + 1),
          "the tile hook");
}

// every (lane, position) of the grid's (lane block, pass, lane of the block, slot of the tile), as k_pos_count derives them
static void cover(int n, int m, int cap) {
    const PosShape s = pos_shape(n, m, cap);
    CHECK(s.tile >= 1 && s.tile <= POS_LDS_QUERIES && s.lanes >= 1 && s.lanes <= n && s.lanes * s.tile <= POS_LDS_QUERIES, "n %d m %d cap %d: the shape", n, m, cap);
    CHECK(cap <= 0 || s.tile <= cap, "n %d m %d cap %d: the cap holds", n, m, cap);
    CHECK(s.lane_blocks >= 1 && s.passes >= 1 && s.lane_blocks <= Q_LANES, "n %d m %d cap %d: the grid", n, m, cap);
    const size_t lds = pos_lds_bytes(s.lanes, s.tile);
    CHECK(lds <= POS_LDS_MAX && POS_LDS_MAX <= 160 * 1024 && 2 * lds <= 160 * 1024, "n %d m %d cap %d: %zu bytes of LDS", n, m, cap, lds);
    CHECK(lds == 16 * (size_t)s.lanes * (size_t)s.tile + 64, "n %d m %d cap %d: keys, ids, slots, counts", n, m, cap);
    CHECK(pos_rows_per_step(s.lanes) >= 1 && pos_rows_per_step(s.lanes) * s.lanes <= POS_BLOCK, "n %d: rows per step", n);
    std::vector<int> seen((size_t)n * (size_t)(m > 0 ? m : 1), 0), counted((size_t)n, 0);
    for (int by = 0; by < s.lane_blocks; ++by)
        for (int bz = 0; bz < s.passes; ++bz) {
            const int l0 = by * s.lanes, nl = std::min(s.lanes, n - l0);
            const int q0 = bz * s.tile, tc = std::max(std::min(s.tile, m - q0), 0);
            CHECK(nl >= 1, "n %d m %d cap %d: an empty lane block", n, m, cap);
            CHECK(m == 0 || tc >= 1, "n %d m %d cap %d: an empty pass", n, m, cap);
            for (int j = 0; j < nl; ++j) {
                if (bz == 0) ++counted[(size_t)(l0 + j)];
                for (int t = 0; t < tc; ++t) ++seen[(size_t)(l0 + j) * (size_t)m + (size_t)(q0 + t)];
            }
        }
    bool once = true;
    for (int i = 0; i < n; ++i) {
        once = once && counted[(size_t)i] == 1;
        for (int q = 0; q < m; ++q) once = once && seen[(size_t)i * (size_t)m + (size_t)q] == 1;
    }
    CHECK(once, "n %d m %d cap %d: every (lane, position) once, every lane counted once", n, m, cap);
    for (int rows : {0, 1, 63, 1024, 100000, 1 << 24}) {
        const int gx = pos_grid_x(rows, s);
        const int per = pos_rows_per_step(s.lanes);
        CHECK(gx >= 1 && (gx == 1 || (long long)(gx - 1) * per < rows), "n %d m %d cap %d rows %d: grid.x %d", n, m, cap, rows, gx);
        CHECK(gx == 1 || (long long)gx * s.lane_blocks * s.passes <= POS_GRID, "n %d m %d cap %d rows %d: the grid's size", n, m, cap, rows);
    }
}

static void shapes() {
    for (int n = 1; n <= Q_LANES; ++n)
        for (int m : {0, 1, 2, 3, 63, 64, 255, 256, 257, 300, 700, 1023, 1365, 1366, 2048, 2049, 4095, 4096})
            for (int cap : {0, 1, 2, 3, 64, 255, 256, 257, 300, 2048, 4095, 4096}) cover(n, m, cap);
    // the two ends the header names: one lane at the largest m, all lanes at a small one
    PosShape s = pos_shape(16, 4096, 0);
    CHECK(s.tile == 4096 && s.lanes == 1 && s.lane_blocks == 16 && s.passes == 1, "16 lanes, 4096 queries");
    s = pos_shape(16, 256, 0);
    CHECK(s.tile == 256 && s.lanes == 16 && s.lane_blocks == 1 && s.passes == 1, "16 lanes, 256 queries");
    s = pos_shape(10, 700, 300);
    CHECK(s.tile == 300 && s.lanes == 10 && s.lane_blocks == 1 && s.passes == 3, "10 lanes, 700 queries, tile 300");
    s = pos_shape(16, 700, 300);
    CHECK(s.tile == 300 && s.lanes == 13 && s.lane_blocks == 2 && s.passes == 3, "16 lanes, 700 queries, tile 300");
    s = pos_shape(10, 0, 0);
    CHECK(s.tile == 1 && s.lanes == 10 && s.lane_blocks == 1 && s.passes == 1, "no query: one pass that counts");
    CHECK(POS_LDS_MAX == 65536 + 64, "one lane of 4096 queries");
}

static void layout() {
    for (int n : {1, 3, 10, 16})
        for (int m : {0, 1, 5, 4096}) {
            const PosWork w = pos_work(n, m);
            CHECK(w.off_key == 0 && w.off_place == 8 * (size_t)n * (size_t)m && w.key_bytes == 12 * (size_t)n * (size_t)m, "n %d m %d: keys and places", n, m);
            CHECK(w.off_place % 8 == 0 && w.slot_elems == (size_t)n * ((size_t)m + 1), "n %d m %d: slots", n, m);
            const PosLayout l = pos_layout(n, m);
            CHECK(l.off_cnt == 0 && l.off_pos == 64 && l.off_pos >= sizeof(int32_t) * Q_LANES && l.total_bytes == 64 + 4 * (size_t)n * (size_t)m, "n %d m %d: the block", n, m);
        }
}

int main() {
    arguments();
    shapes();
    layout();
    std::printf("position plan: %d failures\n", failures);
    return failures ? 1 : 0;
}
