// dppr_export_plan.hpp -- the sizes, the result block and the argument checks of the exports (dppr_support / dppr_export_sparse /
// dppr_export_dense_dev and their group forms). Pure host code without HIP includes (dppr_export.hpp takes the tile from it,
// dppr_host_query.hpp lays the workspace and the staging block out with it and checks a call with it;
// tests/native/export_plan_test.cpp drives it on the CPU against a plain restatement).
//
// WORKSPACE, by the number of external ids V alone (every lane count fits):
//     mask  [V]            16 bits per external id: bit i = lane i qualifies
//     cnt   [tiles][16]    int32: qualifying ids of every lane in every tile of EX_TILE ids
//     base  [tiles][16]    int64: where the tile's first entry of a lane goes (the lane's offset included)
// BLOCK of a sparse export: the head always, the sections only for a host destination (a device destination is written in place):
//     [offsets 17 x int64][go int32, pad]  <- EX_HEAD_BYTES, always copied back
//     [ids cap x int32, padded to 8 bytes][p cap x double][r cap x double, if asked for]
#pragma once

#include "dppr_query_plan.hpp"

namespace dppr {

constexpr int EX_LANES = Q_LANES; // (the name the kernels of dppr_export.hpp know the lane count by)
constexpr int EX_TILE = 256;   // external ids per tile = threads of a workgroup of dppr_export.hpp (4 waves)
constexpr size_t EX_HEAD_BYTES = 8 * (EX_LANES + 1) + 8;

struct ExHead {
    long long offsets[EX_LANES + 1]; // offsets[i] .. offsets[i + 1]: source i; entries past n repeat offsets[n]
    int go;                          // 1: offsets[n] <= cap, the fill ran
    int pad;
};
static_assert(sizeof(ExHead) == EX_HEAD_BYTES, "the head of the block is 17 offsets and the go word");

constexpr int64_t ex_tiles(int64_t V) { return (V + EX_TILE - 1) / EX_TILE; }

struct ExWork {
    size_t mask_elems = 0; // uint16
    size_t cnt_elems = 0;  // int32
    size_t base_elems = 0; // int64
    size_t bytes = 0;
};

constexpr ExWork ex_workspace(int64_t V) {
    ExWork w;
    const size_t tiles = (size_t)(ex_tiles(V) > 0 ? ex_tiles(V) : 1);
    w.mask_elems = (size_t)(V > 0 ? V : 1);
    w.cnt_elems = tiles * EX_LANES;
    w.base_elems = tiles * EX_LANES;
    w.bytes = 2 * w.mask_elems + 4 * w.cnt_elems + 8 * w.base_elems;
    return w;
}

struct ExLayout {
    size_t off_ids = 0, off_p = 0, off_r = 0;
    size_t total_bytes = 0; // head + sections: the device block, the pinned block and the one copy between them
};

// cap entries of a HOST destination (cap = 0, and every device destination: the head alone)
constexpr ExLayout ex_layout(int64_t cap, bool with_r) {
    ExLayout l;
    const size_t c = (size_t)(cap > 0 ? cap : 0);
    l.off_ids = EX_HEAD_BYTES;
    l.off_p = l.off_ids + pad8(sizeof(int32_t) * c);
    l.off_r = l.off_p + sizeof(double) * c;
    l.total_bytes = l.off_r + (with_r ? sizeof(double) * c : 0);
    return l;
}

// no call can return more than one entry per (vertex, source): what a larger cap is worth to the staging block
constexpr int64_t ex_cap_clamped(int64_t cap, int64_t V, int n) { return cap < V * (int64_t)n ? cap : V * (int64_t)n; }

// the arguments of a sparse export that need no device: min_p >= 0 (false for NaN), cap >= 0, a known dest, offsets, and ids / p
// wherever something could be written
inline bool ex_sparse_args_ok(double min_p, int64_t cap, int dest, const void *offsets, const void *ids, const void *p) {
    if (!(min_p >= 0.0) || cap < 0 || (dest != DPPR_DEST_HOST && dest != DPPR_DEST_DEVICE) || !offsets) return false;
    return cap == 0 || (ids && p);
}
inline bool ex_support_args_ok(double min_p, const void *counts) { return min_p >= 0.0 && counts; }

inline bool ex_dense_args_ok(int which, int dtype, int layout) {
    return (which == DPPR_DENSE_P || which == DPPR_DENSE_R) && (dtype == DPPR_F64 || dtype == DPPR_F32) &&
           (layout == DPPR_VERTEX_MAJOR || layout == DPPR_SOURCE_MAJOR);
}

constexpr size_t ex_elem_bytes(int dtype) { return dtype == DPPR_F32 ? 4 : 8; }
// bytes a dense destination must hold, and its alignment (the element size); the same for both layouts
constexpr size_t ex_dense_bytes(int dtype, int n, int64_t V) { return ex_elem_bytes(dtype) * (size_t)n * (size_t)V; }
// element index of (vertex v, source i)
constexpr size_t ex_dense_index(int layout, int n, int64_t V, int64_t v, int i) {
    return layout == DPPR_SOURCE_MAJOR ? (size_t)i * (size_t)V + (size_t)v : (size_t)v * (size_t)n + (size_t)i;
}

// [ptr, ptr + bytes) lies inside the allocation [base, base + size) and ptr is aligned to `align` (a power of two)
inline bool ex_range_ok(uintptr_t ptr, size_t bytes, size_t align, uintptr_t base, size_t size) {
    if (!ptr || (ptr & (uintptr_t)(align - 1)) || ptr < base) return false;
    const uintptr_t at = ptr - base;
    return at <= size && bytes <= size - at;
}

} // namespace dppr
