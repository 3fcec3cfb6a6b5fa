// dppr_ftrack_rank_plan.hpp -- what the ranked, position and sample queries over a forward track (dppr_ftrack_topk_ranked /
// dppr_ftrack_rank_score_at / dppr_ftrack_position_at / dppr_ftrack_sample) decide before any device is involved: the argument
// checks (those of the group forms of dppr_rank_plan.hpp, dppr_position_plan.hpp and dppr_sample_plan.hpp with "lane" read as
// "column"), the seeds of a track's columns as one flat table of EXTERNAL ids, the TILES of the count / fill passes that compact
// the scratch state, the shape of the scan over the tiles' counts, and the sizes of the buffers, 64-bit throughout. Pure host
// code without HIP includes (dppr_host_ftrack_rank.hpp checks a call and lays it out with it, dppr_ftrack_rank.hpp takes its
// constants; tests/native/ftrack_rank_plan_test.cpp drives it on the CPU under the sanitizers).
//
// A CALL on the device:
//     1 mark     (a spec that excludes) one exclusion word per EXTERNAL id, bit c for column c: the seeds' own bits by one thread
//                per seed, the neighbour flags by one wave per piece of a seed's live row (rk_pieces of dppr_rank_plan.hpp)
//     2 count    a tile of `tile_rows` external ids per workgroup, walked in stages of at most FR_STAGE ids: the ids at which at
//                least one column has score > min_score
//     3 scan     the tiles' counts -> the first row of every tile in the compacted scratch state; the total comes to the host ONCE
//     4 fill     the scores recomputed, every kept row placed by its rank inside its tile: the scratch state score[row * m + col]
//                with ext_c[row], in ascending external id
//     5 back     the selection (top k) or the order / count / finish of the positions over the scratch state, as they are.
// The sample needs no compaction (its leaves are by external id already): 1, the leaves, the upper levels, the draws.
#pragma once

#include "dppr_position_plan.hpp"
#include "dppr_sample_plan.hpp"

namespace dppr {

constexpr int FR_BLOCK = 256;                    // threads of every kernel of dppr_ftrack_rank.hpp: four waves
constexpr int FR_WAVES = FR_BLOCK / 64;
constexpr int FR_STAGE = 256;                    // external ids staged in LDS at a time: one per thread
constexpr int FR_LDS_ROW = Q_LANES + 1;          // a staged row, padded by one double (the bank argument of dppr_topk.hpp)
constexpr int FR_TILE_ROWS = 256;                // external ids of a tile on a small window (dppr_debug_ftrack_rank: 64 .. 1024)
constexpr int FR_TILE_ROWS_LARGE = 1024;         // ... from FR_LARGE_V ids on: the one wave of the scan walks a quarter of the tiles, and
constexpr int64_t FR_LARGE_V = (int64_t)1 << 20; //     1024 tiles and more still fill the device (profiles/ftrack_rank_times.md)
constexpr int FR_TILE_MIN = 64, FR_TILE_MAX = 1024;
constexpr int FR_GRID_MAX = 2048;                // workgroups of the count / fill passes: they stride over the tiles
constexpr int FR_SCAN_LANES = 64;                // tiles the one wave of the scan takes per step

// dppr_debug_ftrack_rank: 0 gives the choice back to the plan
constexpr bool fr_tile_ok(int v) { return v == 0 || (v >= FR_TILE_MIN && v <= FR_TILE_MAX && (v & (v - 1)) == 0); }
constexpr int fr_tile_rows(int hook, int64_t V) { return hook ? hook : V >= FR_LARGE_V ? FR_TILE_ROWS_LARGE : FR_TILE_ROWS; }
// ids of a stage (a tile is a whole number of them: both are powers of two)
constexpr int fr_stage_rows(int tile_rows) { return tile_rows < FR_STAGE ? tile_rows : FR_STAGE; }
// LDS of a workgroup: the staged rows, the factor, the exclusion word and the place of every row, the waves' counts
constexpr size_t fr_lds_bytes() { return sizeof(double) * FR_STAGE * FR_LDS_ROW + (sizeof(double) + 2 * sizeof(int)) * FR_STAGE + sizeof(int) * FR_WAVES; }
static_assert(fr_lds_bytes() <= 64 * 1024, "the tile's stage fits the LDS a kernel has without asking");

constexpr int64_t fr_tiles(int64_t V, int tile_rows) { return (V + tile_rows - 1) / tile_rows; }
constexpr int fr_grid(int64_t tiles) { return (int)(tiles < 1 ? 1 : tiles < FR_GRID_MAX ? tiles : FR_GRID_MAX); }
// the first external id of a tile and how many it holds
constexpr int64_t fr_tile_first(int64_t tile, int tile_rows) { return tile * tile_rows; }
constexpr int fr_tile_count(int64_t tile, int64_t V, int tile_rows) {
    const int64_t left = V - fr_tile_first(tile, tile_rows);
    return (int)(left < 0 ? 0 : left < tile_rows ? left : tile_rows);
}
// THE SCAN is k_ex_scan of dppr_export.hpp with one lane: one wave, FR_SCAN_LANES tiles per step with a 32-bit sum inside the step
// and a 64-bit carry between the steps, the tile count an int. What that asks of the tiles:
static_assert((int64_t)FR_TILE_MAX * FR_SCAN_LANES < (1ll << 31), "a step of the scan sums inside an int");
constexpr bool fr_scan_fits(int64_t tiles) { return tiles >= 0 && tiles <= 0x7fffffffll; }
static_assert(fr_scan_fits(fr_tiles(0x7fffffffll, FR_TILE_MIN)), "the tiles of the largest V at the smallest tile count inside an int");

// ---- the seeds of a track's columns ----------------------------------------------------------------------------------------
// one flat table of external ids (FTrack::ids), column c at positions [off[c], off[c + 1]); entries past m repeat off[m]
struct FrSeeds {
    int m = 0;
    int off[Q_LANES + 1] = {0};
    int total() const { return off[Q_LANES]; }
};
inline FrSeeds fr_seeds(const int64_t *offsets /* [m + 1] */, int m) {
    FrSeeds s;
    s.m = m;
    for (int i = 0; i <= Q_LANES; ++i) s.off[i] = (int)offsets[i < m ? i : m];
    return s;
}
// the column that holds position pos (off is non-decreasing: the last column that starts at or before pos; no branch on the data)
constexpr int fr_col_of(const FrSeeds &s, int pos) {
    int c = 0;
    for (int i = 1; i < Q_LANES; ++i) c += pos >= s.off[i] ? 1 : 0;
    return c;
}
// ... as the piece bound of dppr_rank_plan.hpp reads them
inline RkSeeds fr_rk_seeds(const FrSeeds &s) {
    RkSeeds r;
    r.n = s.m;
    for (int i = 0; i <= Q_LANES; ++i) r.off[i] = s.off[i];
    return r;
}

// ---- argument checks: those of the group forms, n = the track's m -------------------------------------------------------------
inline bool fr_topk_args_ok(const dppr_rank_spec_t *s, int32_t k, double min_score, const void *ids, const void *score, const void *cnt) {
    return rank_topk_args_ok(s, k, min_score, ids, score, cnt);
}
inline bool fr_score_at_args_ok(const dppr_rank_spec_t *s, const int32_t *ids, int32_t n_ids, int64_t V, const void *out) {
    return rank_score_at_args_ok(s, ids, n_ids, V, out);
}
inline bool fr_position_args_ok(const dppr_rank_spec_t *s, double min_score, const int32_t *ids, int32_t n_ids, int64_t V, const void *out_pos) {
    return position_args_ok(s, min_score, ids, n_ids, V, out_pos);
}
inline bool fr_sample_args_ok(const dppr_rank_spec_t *s, double min_score, int m, uint64_t first, int64_t S, int dest, const void *out_ids,
                              const void *out_total, const void *out_status) {
    return sample_args_ok(s, min_score, m, first, S, dest, out_ids, out_total, out_status);
}
// a spec that reads a degree or a neighbour needs the track's epoch resident; any other never looks at the graph
inline bool fr_needs_epoch(const dppr_rank_spec_t *s) { return rank_needs_epoch(s); }

// ---- sizes -------------------------------------------------------------------------------------------------------------------
constexpr size_t fr_excl_elems(int64_t V) { return (size_t)(V > 0 ? V : 1); }             // one exclusion word per external id
constexpr size_t fr_seed_elems(int64_t total) { return (size_t)(total > 0 ? total : 1); }
constexpr size_t fr_cnt_elems(int64_t tiles) { return (size_t)(tiles > 0 ? tiles : 1); } // int32 counts, int64 bases
// the compacted scratch state of `rows` kept ids: 8 m + 4 bytes a row
constexpr size_t fr_scratch_bytes(int64_t rows, int m) { return (size_t)rows * (sizeof(double) * (size_t)m + sizeof(int32_t)); }

} // namespace dppr
