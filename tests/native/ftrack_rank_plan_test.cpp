// ftrack_rank_plan_test.cpp -- dynamicppr_amd/csrc/dppr_ftrack_rank_plan.hpp on the CPU: the argument checks of the four calls at
// every limit, the debug hook's values and the plan's choice of a tile, the tiles, stages and grids of the count / fill passes for V
// in {1, 63, 64, 65, 1024, 2^22} at every legal tile_rows -- through fr_tiles / fr_tile_first / fr_tile_count / fr_stage_rows, the
// functions the kernels walk their tiles with: every external id in exactly one tile and one stage --, what the scan (k_ex_scan with
// one lane) asks of the tiles, the seed table of a track's columns with the column of a position as k_fr_mark finds it, and the
// workspace sizes at V = 2^31 - 1, m = 16 without overflow.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_ftrack_rank_plan.hpp"

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

static dppr_rank_spec_t spec(int factor, int dtype, int mask, uint32_t exclude) {
    dppr_rank_spec_t s;
    std::memset(&s, 0, sizeof(s));
    s.factor = factor;
    s.factor_dtype = dtype;
    s.mask = mask;
    s.exclude = exclude;
    return s;
}

static void arguments() {
    int32_t ids[4] = {0, 5, 99, 5}, out_i[4];
    double out_d[4];
    const dppr_rank_spec_t ok = spec(DPPR_FACTOR_INV_DEG, 0, DPPR_MASK_DENY, 7);
    const dppr_rank_spec_t bad[] = {spec(4, 0, 0, 0), spec(-1, 0, 0, 0), spec(DPPR_FACTOR_DEV, 2, 0, 0), spec(0, 0, 3, 0), spec(0, 0, -1, 0), spec(0, 0, 0, 8)};
    const double nan = std::nan("");
    // top k
    CHECK(fr_topk_args_ok(nullptr, 1, 0.0, out_i, out_d, out_i) && fr_topk_args_ok(&ok, DPPR_TOPK_MAX, 1e-4, out_i, out_d, out_i), "the limits themselves");
    CHECK(!fr_topk_args_ok(&ok, 0, 0.0, out_i, out_d, out_i) && !fr_topk_args_ok(&ok, DPPR_TOPK_MAX + 1, 0.0, out_i, out_d, out_i), "k");
    CHECK(!fr_topk_args_ok(&ok, 1, -1e-300, out_i, out_d, out_i) && !fr_topk_args_ok(&ok, 1, nan, out_i, out_d, out_i), "min_score");
    CHECK(!fr_topk_args_ok(&ok, 1, 0.0, nullptr, out_d, out_i) && !fr_topk_args_ok(&ok, 1, 0.0, out_i, nullptr, out_i) &&
              !fr_topk_args_ok(&ok, 1, 0.0, out_i, out_d, nullptr),
          "NULL outputs");
    for (const dppr_rank_spec_t &b : bad) {
        CHECK(!fr_topk_args_ok(&b, 1, 0.0, out_i, out_d, out_i), "a bad spec: topk");
        CHECK(!fr_score_at_args_ok(&b, ids, 4, 100, out_d), "a bad spec: score_at");
        CHECK(!fr_position_args_ok(&b, 0.0, ids, 4, 100, out_i), "a bad spec: position");
        CHECK(!fr_sample_args_ok(&b, 0.0, 1, 0, 1, DPPR_DEST_HOST, out_i, out_d, out_i), "a bad spec: sample");
    }
    // (the dtype is read only for DPPR_FACTOR_DEV)
    const dppr_rank_spec_t odd = spec(DPPR_FACTOR_DEG, 9, 0, 0);
    CHECK(fr_topk_args_ok(&odd, 1, 0.0, out_i, out_d, out_i), "a dtype nobody reads");
    // scores at ids
    CHECK(fr_score_at_args_ok(&ok, ids, 4, 100, out_d) && fr_score_at_args_ok(nullptr, nullptr, 0, 100, out_d), "score_at: fine");
    CHECK(!fr_score_at_args_ok(&ok, ids, 4, 99, out_d) && !fr_score_at_args_ok(&ok, ids, -1, 100, out_d) && !fr_score_at_args_ok(&ok, nullptr, 4, 100, out_d) &&
              !fr_score_at_args_ok(&ok, ids, 4, 100, nullptr),
          "score_at: an id outside [0, V), n_ids < 0, NULL ids, NULL out");
    // positions
    CHECK(fr_position_args_ok(&ok, 0.0, ids, 4, 100, out_i) && fr_position_args_ok(nullptr, 0.5, nullptr, 0, 100, nullptr), "position: fine");
    CHECK(!fr_position_args_ok(&ok, 0.0, ids, -1, 100, out_i) && !fr_position_args_ok(&ok, 0.0, ids, DPPR_POSITION_MAX + 1, 1 << 20, out_i), "position: n_ids");
    CHECK(!fr_position_args_ok(&ok, 0.0, ids, 4, 99, out_i) && !fr_position_args_ok(&ok, -1.0, ids, 4, 100, out_i) && !fr_position_args_ok(&ok, nan, ids, 4, 100, out_i) &&
              !fr_position_args_ok(&ok, 0.0, nullptr, 4, 100, out_i) && !fr_position_args_ok(&ok, 0.0, ids, 4, 100, nullptr),
          "position: ids, min_score, NULLs");
    // samples
    CHECK(fr_sample_args_ok(&ok, 0.0, 16, 0, DPPR_SAMPLE_MAX, DPPR_DEST_DEVICE, out_i, out_d, out_i), "sample: 16 x 2^20 is the total's limit");
    CHECK(fr_sample_args_ok(nullptr, 0.0, 1, ~0ull, 0, DPPR_DEST_HOST, nullptr, out_d, out_i), "sample: S == 0 needs no ids");
    CHECK(!fr_sample_args_ok(&ok, 0.0, 1, 0, DPPR_SAMPLE_MAX + 1, 0, out_i, out_d, out_i) && !fr_sample_args_ok(&ok, 0.0, 1, 0, -1, 0, out_i, out_d, out_i), "sample: S");
    CHECK(!fr_sample_args_ok(&ok, 0.0, 1, ~0ull, 1, 0, out_i, out_d, out_i) && fr_sample_args_ok(&ok, 0.0, 1, ~0ull - 1, 1, 0, out_i, out_d, out_i), "sample: first + S wraps");
    CHECK(!fr_sample_args_ok(&ok, 0.0, 1, 0, 1, 2, out_i, out_d, out_i) && !fr_sample_args_ok(&ok, -1.0, 1, 0, 1, 0, out_i, out_d, out_i) &&
              !fr_sample_args_ok(&ok, nan, 1, 0, 1, 0, out_i, out_d, out_i),
          "sample: dest, min_score");
    CHECK(!fr_sample_args_ok(&ok, 0.0, 1, 0, 1, 0, nullptr, out_d, out_i) && !fr_sample_args_ok(&ok, 0.0, 1, 0, 1, 0, out_i, nullptr, out_i) &&
              !fr_sample_args_ok(&ok, 0.0, 1, 0, 1, 0, out_i, out_d, nullptr),
          "sample: NULLs");
    // the epoch rule
    const dppr_rank_spec_t dev = spec(DPPR_FACTOR_DEV, 1, DPPR_MASK_ALLOW, DPPR_EXCLUDE_SEEDS);
    CHECK(!fr_needs_epoch(nullptr) && !fr_needs_epoch(&dev), "no degree, no neighbour: the graph is never looked at");
    const dppr_rank_spec_t deg = spec(DPPR_FACTOR_DEG, 0, 0, 0), inv = spec(DPPR_FACTOR_INV_DEG, 0, 0, 0), in = spec(0, 0, 0, DPPR_EXCLUDE_IN_NEIGHBOURS),
                           out = spec(0, 0, 0, DPPR_EXCLUDE_OUT_NEIGHBOURS);
    CHECK(fr_needs_epoch(&deg) && fr_needs_epoch(&inv) && fr_needs_epoch(&in) && fr_needs_epoch(&out), "degrees and neighbours need the track's epoch");
    // the hook
    CHECK(fr_tile_ok(0) && fr_tile_ok(64) && fr_tile_ok(128) && fr_tile_ok(256) && fr_tile_ok(512) && fr_tile_ok(1024), "the hook's values");
    CHECK(!fr_tile_ok(32) && !fr_tile_ok(2048) && !fr_tile_ok(96) && !fr_tile_ok(-64) && !fr_tile_ok(1), "... and what it refuses");
    CHECK(fr_tile_rows(0, 1024) == FR_TILE_ROWS && fr_tile_rows(0, FR_LARGE_V - 1) == 256 && fr_tile_rows(0, FR_LARGE_V) == 1024 &&
              fr_tile_rows(0, ((int64_t)1 << 31) - 1) == FR_TILE_ROWS_LARGE && fr_tile_rows(64, (int64_t)1 << 22) == 64 && fr_tile_rows(1024, 1) == 1024,
          "0: the plan decides, by V");
    CHECK(fr_tiles(FR_LARGE_V, fr_tile_rows(0, FR_LARGE_V)) == 1024, "a large window has 1024 tiles and more");
}

static void tiles() {
    const int64_t Vs[] = {1, 63, 64, 65, 1024, (int64_t)1 << 22};
    for (int64_t V : Vs)
        for (int tr = FR_TILE_MIN; tr <= FR_TILE_MAX; tr *= 2) {
            const int64_t t = fr_tiles(V, tr);
            CHECK(t == (V + tr - 1) / tr && t >= 1, "tiles V=%" PRId64 " tr=%d", V, tr);
            CHECK(fr_grid(t) >= 1 && fr_grid(t) <= FR_GRID_MAX && fr_grid(t) <= t, "grid V=%" PRId64 " tr=%d", V, tr);
            const int stage = fr_stage_rows(tr);
            CHECK(stage <= FR_STAGE && stage <= tr && tr % stage == 0, "stages tr=%d", tr);
            // every external id lies in exactly one tile and one stage of it, in ascending order
            int64_t covered = 0;
            bool in_order = true;
            for (int64_t tile = 0; tile < t; ++tile) {
                const int64_t first = fr_tile_first(tile, tr);
                const int cnt = fr_tile_count(tile, V, tr);
                in_order = in_order && first == covered && cnt >= 1 && cnt <= tr;
                int staged = 0;
                for (int64_t e0 = first; e0 < first + cnt; e0 += stage) staged += (int)std::min<int64_t>(stage, first + cnt - e0);
                in_order = in_order && staged == cnt;
                covered += cnt;
            }
            CHECK(in_order && covered == V, "cover V=%" PRId64 " tr=%d covered=%" PRId64, V, tr, covered);
            CHECK(fr_tile_count(t, V, tr) == 0, "a tile past the end holds nothing");
        }
    CHECK(fr_grid(0) == 1 && fr_grid(1) == 1 && fr_grid(FR_GRID_MAX) == FR_GRID_MAX && fr_grid((int64_t)1 << 25) == FR_GRID_MAX, "the grid's bounds");
    CHECK(fr_lds_bytes() == 8u * 256 * 17 + 16u * 256 + 16u && fr_lds_bytes() <= 64u * 1024, "the stage's LDS: %zu", fr_lds_bytes());
}

static void scan() {
    // k_ex_scan counts its tiles in an int, sums 64 counts of a step in an int and carries 64 bits between the steps
    CHECK(fr_scan_fits(0) && fr_scan_fits(1) && fr_scan_fits(0x7fffffffll) && !fr_scan_fits(0x80000000ll) && !fr_scan_fits(-1), "the tile count is an int");
    for (int tr = FR_TILE_MIN; tr <= FR_TILE_MAX; tr *= 2) CHECK(fr_scan_fits(fr_tiles(0x7fffffffll, tr)), "the largest V at tile_rows %d", tr);
    CHECK((int64_t)FR_TILE_MAX * FR_SCAN_LANES < ((int64_t)1 << 31), "a step inside an int");
    CHECK(fr_tiles(0x7fffffffll, FR_TILE_MIN) * (int64_t)FR_TILE_MIN > 0x7fffffffll - FR_TILE_MIN, "every tile full: the total needs the 64-bit carry's room only at the end");
}

static void seeds() {
    const int64_t off[] = {0, 1, 1, 4, 4100};
    const FrSeeds s = fr_seeds(off, 4);
    CHECK(s.m == 4 && s.total() == 4100 && s.off[0] == 0 && s.off[1] == 1 && s.off[2] == 1 && s.off[3] == 4 && s.off[4] == 4100 && s.off[5] == 4100 &&
              s.off[Q_LANES] == 4100,
          "offsets, repeated past m");
    CHECK(fr_col_of(s, 0) == 0 && fr_col_of(s, 1) == 2 && fr_col_of(s, 3) == 2 && fr_col_of(s, 4) == 3 && fr_col_of(s, 4099) == 3, "the column of a position (an empty column owns none)");
    const RkSeeds r = fr_rk_seeds(s);
    CHECK(r.n == 4 && r.total() == 4100 && rk_lane_of(r, 4) == 3 && rk_lane_of(r, 1) == 2, "as the piece bound reads them");
    int64_t full[Q_LANES + 1];
    for (int i = 0; i <= Q_LANES; ++i) full[i] = (int64_t)i * DPPR_FPUSH_SET_MAX;
    const FrSeeds f = fr_seeds(full, Q_LANES);
    CHECK(f.total() == Q_LANES * DPPR_FPUSH_SET_MAX && fr_col_of(f, 0) == 0 && fr_col_of(f, 4095) == 0 && fr_col_of(f, 4096) == 1 && fr_col_of(f, 65535) == 15,
          "16 x 4096 at the most");
    for (int pos = 0; pos < s.total(); pos += 7) CHECK(fr_col_of(s, pos) == rk_lane_of(r, pos), "one column rule for the marking and the piece bound: %d", pos);
}

static void sizes() {
    const int64_t V = ((int64_t)1 << 31) - 1;
    CHECK(fr_excl_elems(V) == (size_t)V && fr_excl_elems(0) == 1, "exclusion words");
    CHECK(fr_tiles(V, FR_TILE_MIN) == (int64_t)1 << 25 && fr_cnt_elems(fr_tiles(V, FR_TILE_MIN)) == (size_t)1 << 25 && fr_cnt_elems(0) == 1, "tiles at the largest V");
    CHECK(fr_scratch_bytes(V, 16) == (size_t)V * 132 && fr_scratch_bytes(V, 16) > ((size_t)1 << 38), "scratch: 8 m + 4 bytes a row, 64-bit: %zu", fr_scratch_bytes(V, 16));
    CHECK(fr_scratch_bytes(0, 16) == 0 && fr_scratch_bytes(10, 1) == 120, "scratch: small");
    CHECK(scratch_plane_elems((size_t)V, 16) == (size_t)V * 16 && scratch_ext_elems((size_t)V) == (size_t)V, "the scratch state's own arithmetic");
    CHECK(sample_leaf_elems(16, sample_tree(V).Vt) == (size_t)16 << 31, "a sample's leaves at the largest V");
    CHECK(pos_work(16, DPPR_POSITION_MAX).key_bytes == 12u * 16 * 4096, "a position call's keys");
    CHECK(fr_seed_elems(0) == 1 && fr_seed_elems(65536) == 65536, "seed table");
}

int main() {
    arguments();
    tiles();
    scan();
    seeds();
    sizes();
    std::printf("ftrack_rank_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
