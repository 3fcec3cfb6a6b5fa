// dppr_dot_plan.hpp -- the sizes, the tile table, the result head and the argument checks of the dot products over the vertex
// axis (dppr_dot_dense_dev / dppr_dot_sparse and their group forms), and a plain host restatement of their fold. Pure host code
// without HIP includes (dppr_dot.hpp takes the tile constants from it, dppr_host_query.hpp lays the workspace out with it and checks
// a call with it; tests/native/dot_plan_test.cpp drives it on the CPU).
//
// THE FOLD (include/dppr.h states it): slots in blocks of DOT_BLOCK = 2^16, a block summed by the balanced binary tree that adds
// neighbours, missing slots of the last block +0.0, the blocks added in ascending order. The device realises one tree in three
// pieces, every piece a power of two of the one below, so the pieces ARE that tree:
//     subtile   DOT_TILE = 256 slots        staged in LDS, one workgroup step
//     tile      DOT_SUB  = 8 subtiles       one workgroup, combined in registers: ONE partial per (tile, output) leaves the pass
//     block     DOT_TPB  = 32 tiles         the combine launch: tree over the 32 partials, then the running sum over the blocks
// PARTIALS, output-major: part[o * stride + t], stride a multiple of DOT_TPB, zeroed (+0.0) before the pass so that the tiles of
// padding are there without being written.
//     dense    o = (f - f0) * n + i for the features [f0, f0 + launch features) of one launch; t = tile of external ids
//     sparse   o = i; t = col[f] + (tile of query f), col[f] a multiple of DOT_TPB: every query begins a block of its own
// BLOCK of a call: [DotHead][out F x n doubles, only for a host destination]; device and pinned host.
#pragma once

#include <vector>

#include "dppr_query_plan.hpp"

namespace dppr {

constexpr int DOT_TILE = 256;                        // slots of a subtile = threads of a workgroup of dppr_dot.hpp
constexpr int DOT_SUB = 8;                           // subtiles of a tile
constexpr int DOT_WG_SLOTS = DOT_TILE * DOT_SUB;     // slots of a tile: 2048
constexpr int64_t DOT_BLOCK = 1 << 16;               // slots of a block of the fold
constexpr int DOT_TPB = (int)(DOT_BLOCK / DOT_WG_SLOTS); // tiles of a block: 32
constexpr int DOT_FCHUNK = 16;                       // features one workgroup folds against a gathered row
constexpr size_t DOT_PART_BUDGET = (size_t)64 << 20; // bytes of partials one dense launch may fill (a launch takes fewer features instead)
constexpr size_t DOT_HEAD_BYTES = 8;
static_assert((DOT_TILE & (DOT_TILE - 1)) == 0 && (DOT_SUB & (DOT_SUB - 1)) == 0 && (DOT_TPB & (DOT_TPB - 1)) == 0 &&
                  (int64_t)DOT_TILE * DOT_SUB * DOT_TPB == DOT_BLOCK,
              "subtile, tile and block are powers of two of one another: the pieces are one balanced tree");

struct DotHead {
    int bad; // 1: an id of a sparse call in device memory lay outside [0, V): the combine launch wrote nothing
    int pad;
};
static_assert(sizeof(DotHead) == DOT_HEAD_BYTES, "the head of the block is the flag and a pad word");

// one tile of a sparse call: entries [e0, e0 + cnt) of ids / w, partial column `col`
struct DotTile {
    long long e0;
    long long col;
    int cnt; // 1 .. DOT_WG_SLOTS
    int pad;
};
static_assert(sizeof(DotTile) == 24, "a tile of the table is 24 bytes");

constexpr int64_t dot_tiles(int64_t slots) { return (slots + DOT_WG_SLOTS - 1) / DOT_WG_SLOTS; }
constexpr int64_t dot_blocks(int64_t slots) { return (slots + DOT_BLOCK - 1) / DOT_BLOCK; }
// partial columns of `slots` slots: whole blocks
constexpr int64_t dot_cols(int64_t slots) { return dot_blocks(slots) * DOT_TPB; }

constexpr size_t dot_elem_bytes(int dtype) { return dtype == DPPR_F32 ? 4 : 8; }
constexpr size_t dot_dense_h_bytes(int dtype, int F, int64_t V) { return dot_elem_bytes(dtype) * (size_t)F * (size_t)V; }
constexpr size_t dot_h_index(int layout, int F, int64_t V, int f, int64_t v) {
    return layout == DPPR_H_VERTEX_MAJOR ? (size_t)v * (size_t)F + (size_t)f : (size_t)f * (size_t)V + (size_t)v;
}
constexpr size_t dot_out_bytes(int F, int n) { return sizeof(double) * (size_t)F * (size_t)n; }
// the block: the head, and the results of a host destination
constexpr size_t dot_block_bytes(int F, int n, int dest) { return DOT_HEAD_BYTES + (dest == DPPR_DEST_HOST ? dot_out_bytes(F, n) : 0); }

// features of one dense launch: whole chunks of DOT_FCHUNK, as many as the budget of partials holds, one chunk at the least
constexpr int dot_launch_features(int64_t V, int n, int F) {
    const size_t per_feature = sizeof(double) * (size_t)n * (size_t)(dot_cols(V) > 0 ? dot_cols(V) : DOT_TPB);
    size_t f = DOT_PART_BUDGET / per_feature / DOT_FCHUNK * DOT_FCHUNK;
    if (f < (size_t)DOT_FCHUNK) f = DOT_FCHUNK;
    return f < (size_t)F ? (int)f : F;
}
// doubles of the partials of a dense call
constexpr size_t dot_dense_part_elems(int64_t V, int n, int F) {
    return (size_t)dot_launch_features(V, n, F) * (size_t)n * (size_t)(dot_cols(V) > 0 ? dot_cols(V) : DOT_TPB);
}
// slot groups of a subtile: the largest power of two G with G * outputs <= DOT_TILE (every group folds a subtree of DOT_TILE / G slots)
constexpr int dot_groups(int outputs) {
    int g = 1;
    while (2 * g * outputs <= DOT_TILE) g *= 2;
    return g;
}
// dynamic LDS of a pass: rows [DOT_TILE][gw + 1], h [fc][DOT_TILE + 1], partials [DOT_TILE] (doubles), row ids [DOT_TILE] (int)
constexpr size_t dot_lds_bytes(int gw, int fc) {
    return sizeof(double) * ((size_t)DOT_TILE * (gw + 1) + (size_t)fc * (DOT_TILE + 1) + DOT_TILE) + sizeof(int) * DOT_TILE;
}

inline bool dot_enums_ok(int which, int dest) {
    return (which == DPPR_DENSE_P || which == DPPR_DENSE_R) && (dest == DPPR_DEST_HOST || dest == DPPR_DEST_DEVICE);
}
inline bool dot_f_ok(int F) { return F >= 1 && F <= DPPR_DOT_MAX_F; }
inline bool dot_dense_args_ok(int which, const void *h, int dtype, int layout, int F, int dest, const void *out) {
    return dot_enums_ok(which, dest) && dot_f_ok(F) && h && out && (dtype == DPPR_F64 || dtype == DPPR_F32) &&
           (layout == DPPR_H_FEATURE_MAJOR || layout == DPPR_H_VERTEX_MAJOR);
}
// offsets [F + 1]: offsets[0] = 0, non-decreasing
inline bool dot_offsets_ok(const int64_t *offsets, int F) {
    if (!offsets || offsets[0] != 0) return false;
    for (int f = 0; f < F; ++f)
        if (offsets[f + 1] < offsets[f]) return false;
    return true;
}
inline bool dot_sparse_args_ok(int which, const int64_t *offsets, const void *ids, const void *w, int src, int F, int dest,
                               const void *out) {
    return dot_enums_ok(which, dest) && dot_f_ok(F) && (src == DPPR_DEST_HOST || src == DPPR_DEST_DEVICE) && ids && w && out &&
           dot_offsets_ok(offsets, F);
}

// The tile table of a sparse call from its (checked) host offsets: col[f] .. col[f + 1] are query f's partial columns (whole blocks:
// an empty query has none), tiles in query order, a query's tiles in slot order.
struct DotTable {
    std::vector<long long> col; // [F + 1]
    std::vector<DotTile> tiles;
    long long cols() const { return col.empty() ? 0 : col.back(); }
};

inline void dot_table_counts(const int64_t *offsets, int F, long long *n_tiles, long long *n_cols) {
    long long t = 0, c = 0;
    for (int f = 0; f < F; ++f) {
        const int64_t m = offsets[f + 1] - offsets[f];
        t += dot_tiles(m);
        c += dot_cols(m);
    }
    *n_tiles = t;
    *n_cols = c;
}

inline void dot_tile_table(const int64_t *offsets, int F, DotTable &tb) {
    long long n_tiles = 0, n_cols = 0;
    dot_table_counts(offsets, F, &n_tiles, &n_cols);
    tb.col.assign((size_t)F + 1, 0);
    tb.tiles.clear();
    tb.tiles.reserve((size_t)n_tiles);
    long long c = 0;
    for (int f = 0; f < F; ++f) {
        tb.col[(size_t)f] = c;
        const int64_t m = offsets[f + 1] - offsets[f];
        for (int64_t k = 0; k < dot_tiles(m); ++k) {
            DotTile t;
            t.e0 = offsets[f] + k * DOT_WG_SLOTS;
            t.col = c + k;
            t.cnt = (int)(m - k * DOT_WG_SLOTS < DOT_WG_SLOTS ? m - k * DOT_WG_SLOTS : DOT_WG_SLOTS);
            t.pad = 0;
            tb.tiles.push_back(t);
        }
        c += dot_cols(m);
    }
    tb.col[(size_t)F] = c;
}

// bytes of the device input of a sparse call: [tiles][col, padded to 8][ids of a host source, padded to 8][w of a host source]
struct DotSparseWork {
    size_t off_col = 0, off_ids = 0, off_w = 0, bytes = 0;
};
constexpr DotSparseWork dot_sparse_work(long long n_tiles, int F, int64_t m, bool host_src) {
    DotSparseWork w;
    w.off_col = sizeof(DotTile) * (size_t)n_tiles;
    w.off_ids = w.off_col + sizeof(long long) * ((size_t)F + 1);
    w.off_w = w.off_ids + (host_src ? pad8(sizeof(int32_t) * (size_t)m) : 0);
    w.bytes = w.off_w + (host_src ? sizeof(double) * (size_t)m : 0);
    if (w.bytes < 8) w.bytes = 8;
    return w;
}

// The fold of include/dppr.h over m terms, restated plainly: pad the last block, halve level by level, add the blocks in order.
// (volatile: every sum is rounded to double where it stands, whatever the host compiler would like to keep wider)
inline double dot_fold_ref(const double *t, int64_t m) {
    if (m <= 0) return 0.0;
    std::vector<double> y((size_t)DOT_BLOCK);
    double acc = 0.0;
    for (int64_t b = 0; b < dot_blocks(m); ++b) {
        for (int64_t j = 0; j < DOT_BLOCK; ++j) y[(size_t)j] = b * DOT_BLOCK + j < m ? t[b * DOT_BLOCK + j] : 0.0;
        for (int64_t len = DOT_BLOCK; len > 1; len /= 2)
            for (int64_t j = 0; j < len / 2; ++j) {
                volatile double s = y[(size_t)(2 * j)] + y[(size_t)(2 * j + 1)];
                y[(size_t)j] = s;
            }
        if (b == 0) {
            acc = y[0];
        } else {
            volatile double s = acc + y[0];
            acc = s;
        }
    }
    return acc;
}

} // namespace dppr
