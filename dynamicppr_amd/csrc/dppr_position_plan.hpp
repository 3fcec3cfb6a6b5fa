// dppr_position_plan.hpp -- what the position queries (dppr_position_at / dppr_group_position_at) decide before any device is
// involved: the check of a call's arguments, the SHAPE of the count pass -- how many of a lane's ordered queries a workgroup holds
// in LDS per pass (the tile), how many lanes it serves beside each other, and with them the lane blocks and the passes of the grid
// -- the LDS that shape takes, the layout of the workspace and of the result block. Pure host code without HIP includes
// (dppr_host_query.hpp checks a call and lays it out with it, dppr_position.hpp asserts its constants;
// tests/native/position_plan_test.cpp drives it on the CPU under the sanitizers).
//
// SHAPE. A workgroup of k_pos_count holds, for each of its `lanes` lanes, `tile` consecutive queries of that lane's order: a key of
// 8 bytes, an id of 4 and a histogram slot of 4, and one counter per lane. lanes x tile never exceeds POS_LDS_QUERIES = 4096, so
// the LDS of a workgroup is 64 KiB + 64 bytes at the most and a CU (160 KiB) holds two workgroups: one lane at tile = 4096, all 16
// at tile <= 256. blockIdx.y walks the lane blocks, blockIdx.z the passes; a (lane, position in the lane's order) pair belongs to
// exactly one (lane block, pass, slot of the tile).
// WORKSPACE. [n][m] keys of 8 bytes, then [n][m] places of 4 (the permutation: the place in `ids` of every position of the order);
// [n][m + 1] slots of 4 bytes, slot m of a lane being its count of qualifying rows.
// BLOCK, one copy to the host:  [16 counts] <- POS_OFF_POS = 64 bytes  [pos m x n, vertex-major like the state]
#pragma once

#include "dppr_rank_plan.hpp"

namespace dppr {

constexpr int POS_BLOCK = 1024;       // k_pos_count, k_pos_finish: sixteen waves
constexpr int POS_ORDER_BLOCK = 256;  // k_pos_order: one query per thread, the lane's queries in LDS
constexpr int POS_LDS_QUERIES = 4096; // (lane, query) pairs a workgroup of k_pos_count holds
constexpr int POS_SLOT_BYTES = 16;    // ... each a key (8), an id (4) and a histogram slot (4)
constexpr int POS_GRID = 512;         // workgroups of k_pos_count a call aims at: two per CU
static_assert(POS_LDS_QUERIES == DPPR_POSITION_MAX, "one lane at the largest m is one pass");

inline bool position_args_ok(const dppr_rank_spec_t *s, double min_score, const int32_t *ids, int32_t m, int64_t V, const void *out_pos) {
    if (!rank_spec_ok(s) || !(min_score >= 0.0)) return false; // (min_score >= 0 is false for NaN)
    if (m < 0 || m > DPPR_POSITION_MAX) return false;
    if (m > 0 && (!ids || !out_pos)) return false;
    return ids_in_range(ids, m, V);
}
// dppr_debug_position_tile: 0 gives the choice back to the plan
inline bool position_tile_ok(int queries) { return queries >= 0 && queries <= DPPR_POSITION_MAX; }

struct PosShape {
    int tile = 1;        // queries of a lane's order a workgroup holds per pass
    int lanes = 1;       // lanes a workgroup serves
    int lane_blocks = 1; // grid.y
    int passes = 1;      // grid.z
};
// n lanes, m queries, cap: dppr_debug_position_tile (0: none)
constexpr PosShape pos_shape(int n, int m, int cap) {
    PosShape s;
    s.tile = m < 1 ? 1 : m;
    if (cap > 0 && s.tile > cap) s.tile = cap;
    if (s.tile > POS_LDS_QUERIES) s.tile = POS_LDS_QUERIES;
    s.lanes = POS_LDS_QUERIES / s.tile;
    if (s.lanes > n) s.lanes = n;
    s.lane_blocks = (n + s.lanes - 1) / s.lanes;
    s.passes = m < 1 ? 1 : (m + s.tile - 1) / s.tile; // (m == 0: one pass that only counts)
    return s;
}
constexpr size_t pos_lds_bytes(int lanes, int tile) { return (size_t)POS_SLOT_BYTES * (size_t)lanes * (size_t)tile + sizeof(unsigned) * Q_LANES; }
constexpr size_t POS_LDS_MAX = pos_lds_bytes(1, POS_LDS_QUERIES);
static_assert(POS_LDS_MAX <= 160 * 1024 / 2, "two workgroups of k_pos_count share the 160 KiB of a CU");
// rows of the scratch state a workgroup reads per step: thread t serves lane t % lanes of row t / lanes
constexpr int pos_rows_per_step(int lanes) { return POS_BLOCK / lanes; }
// grid.x: a workgroup per step at the most, POS_GRID workgroups over all lane blocks and passes at the most
constexpr int pos_grid_x(int rows, const PosShape &s) {
    const int per = pos_rows_per_step(s.lanes);
    int steps = (rows + per - 1) / per;
    if (steps < 1) steps = 1;
    int share = POS_GRID / (s.lane_blocks * s.passes);
    if (share < 1) share = 1;
    return steps < share ? steps : share;
}

struct PosWork {
    size_t off_key = 0, off_place = 0; // into the key buffer (bytes)
    size_t key_bytes = 0;              // 12 m n
    size_t slot_elems = 0;             // (m + 1) n
};
constexpr PosWork pos_work(int n, int m) {
    PosWork w;
    const size_t nm = (size_t)n * (size_t)m;
    w.off_place = sizeof(unsigned long long) * nm;
    w.key_bytes = w.off_place + sizeof(int32_t) * nm;
    w.slot_elems = (size_t)n * ((size_t)m + 1);
    return w;
}

constexpr size_t POS_OFF_POS = 64; // the 16 counts come first
struct PosLayout {
    size_t off_cnt = 0, off_pos = POS_OFF_POS;
    size_t total_bytes = 0;
};
constexpr PosLayout pos_layout(int n, int m) {
    PosLayout l;
    l.total_bytes = l.off_pos + sizeof(int32_t) * (size_t)n * (size_t)m;
    return l;
}

} // namespace dppr
