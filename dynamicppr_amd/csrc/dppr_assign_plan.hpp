// dppr_assign_plan.hpp -- what dppr_assign / dppr_assign_at decide before any device is involved: the argument checks, the class
// table of a call (the lanes of its groups, concatenated in call order), the team of lanes that reads one vertex, tile counts,
// workspace sizes and the layout of the result block. Pure host code without HIP includes (dppr_assign.hpp takes the tile, the
// head and the group descriptors from it, dppr_host_query.hpp checks a call and lays its workspace and block out with it;
// tests/native/assign_plan_test.cpp drives it on the CPU against a plain restatement).
//
// WORKSPACE, by the number of external ids V alone:
//     cnt   [tiles]            int32: flips of every tile of AS_TILE ids
//     base  [tiles]            int32: where the tile's first flip goes
//     ws    [3][tiles x 256]   int32: id | old | new of every tile's flips, compacted inside the tile in id order
//     scale [256]              double: the scales of the call
// BLOCK: the head always, the sections only for a host destination (a device destination is written in place):
//     [n_flips int64][go int32, pad][counts 257 x int64]  <- AS_HEAD_BYTES, always copied back
//     [label V x int32, padded to 8 bytes][best V x double, if asked for][margin V x double, if asked for]
//     [flip_id cap x int32, padded][flip_old cap x int32, padded][flip_new cap x int32, padded]
// A host destination's prev_label is copied INTO the label section and updated there in place.
#pragma once

#include "dppr_query_plan.hpp"

namespace dppr {

constexpr int AS_GROUPS_MAX = DPPR_ASSIGN_GROUPS_MAX;
constexpr int AS_CLASSES_MAX = DPPR_ASSIGN_CLASSES_MAX;
constexpr int AS_TILE = 256;     // external ids per tile = threads of a workgroup of dppr_assign.hpp (4 waves)
constexpr int AS_TEAM_MAX = 8;   // lanes that read one vertex's rows, 16 bytes each: a 128-byte row in one instruction
static_assert(AS_GROUPS_MAX * Q_LANES == AS_CLASSES_MAX, "16 groups of 16 lanes are the 256 classes");

struct AsHead {
    long long n_flips;                    // the TRUE number of flips (0 without prev_label)
    int go;                               // 1: n_flips <= cap, the fill ran
    int pad;
    long long counts[AS_CLASSES_MAX + 1]; // counts[c]: vertices labelled c; counts[C]: unassigned; entries past C are 0
};
constexpr size_t AS_HEAD_BYTES = 16 + 8 * (AS_CLASSES_MAX + 1);
static_assert(sizeof(AsHead) == AS_HEAD_BYTES, "the head of the block is the flip count, the go word and 257 counts");

// one group of a call as the kernels see it (by value, as a kernel argument): its p rows, their width, lanes in use, first class
struct AsGroup {
    const double *p;
    int gw, n, base;
};
struct AsDesc {
    AsGroup g[AS_GROUPS_MAX];
    int n_groups, C;
};

constexpr int64_t as_tiles(int64_t V) { return (V + AS_TILE - 1) / AS_TILE; }

// The class table of a call: n[i] lanes of the i-th named group -> its first class; C in total. ok: n_groups in range, every
// n[i] in [1, 16] and C <= 256 (always true then: 16 x 16; kept as a check of its own for a wider group one day).
struct AsTable {
    int base[AS_GROUPS_MAX] = {0};
    int C = 0;
    bool ok = false;
};
inline AsTable as_table(const int *n, int n_groups) {
    AsTable t;
    if (!n || n_groups < 1 || n_groups > AS_GROUPS_MAX) return t;
    for (int i = 0; i < n_groups; ++i) {
        if (n[i] < 1 || n[i] > Q_LANES) return t;
        t.base[i] = t.C;
        t.C += n[i];
    }
    t.ok = t.C <= AS_CLASSES_MAX;
    return t;
}

// lanes per vertex: the smallest power of two that reads the widest row of the call (gw doubles) as 16-byte pieces in one step
constexpr int as_team(int max_gw) {
    int t = 1;
    while (t < AS_TEAM_MAX && 2 * t < max_gw) t *= 2;
    return t;
}

struct AsWork {
    size_t cnt_elems = 0, base_elems = 0; // int32
    size_t ws_elems = 0;                  // int32: three planes of ws_plane each
    size_t ws_plane = 0;
    size_t scale_elems = AS_CLASSES_MAX;  // double
    size_t bytes = 0;
};
constexpr AsWork as_workspace(int64_t V) {
    AsWork w;
    const size_t tiles = (size_t)(as_tiles(V) > 0 ? as_tiles(V) : 1);
    w.cnt_elems = w.base_elems = tiles;
    w.ws_plane = tiles * AS_TILE;
    w.ws_elems = 3 * w.ws_plane;
    w.bytes = 4 * (w.cnt_elems + w.base_elems + w.ws_elems) + 8 * w.scale_elems;
    return w;
}

// no call has more flips than vertices: what a larger cap is worth to the block and to a destination's range check
constexpr int64_t as_cap_clamped(int64_t cap, int64_t V) { return cap < V ? cap : V; }

struct AsLayout {
    size_t off_label = 0, off_best = 0, off_margin = 0, off_fid = 0, off_fold = 0, off_fnew = 0;
    size_t total_bytes = 0; // head + sections: the device block, the pinned block and the one copy between them
};
// host = false (a device destination): the head alone, every offset at its end
constexpr AsLayout as_layout(int64_t V, int64_t cap, bool with_best, bool with_margin, bool host) {
    AsLayout l;
    const size_t v = host && V > 0 ? (size_t)V : 0, c = host && cap > 0 ? (size_t)cap : 0;
    l.off_label = AS_HEAD_BYTES;
    l.off_best = l.off_label + pad8(sizeof(int32_t) * v);
    l.off_margin = l.off_best + (with_best ? sizeof(double) * v : 0);
    l.off_fid = l.off_margin + (with_margin ? sizeof(double) * v : 0);
    l.off_fold = l.off_fid + pad8(sizeof(int32_t) * c);
    l.off_fnew = l.off_fold + pad8(sizeof(int32_t) * c);
    l.total_bytes = l.off_fnew + pad8(sizeof(int32_t) * c);
    return l;
}

// The arguments of both calls that need no device, rule by rule (the first that fails)
enum AsCheck {
    AS_OK = 0,
    AS_BAD_GROUPS,   // groups NULL or n_groups outside [1, DPPR_ASSIGN_GROUPS_MAX]
    AS_BAD_SCALE,    // a scale that is not finite or is negative
    AS_BAD_MIN,      // min_score negative or NaN
    AS_BAD_DEST,     // dest neither DPPR_DEST_HOST nor DPPR_DEST_DEVICE
    AS_NULL_OUT,     // out_label or out_counts NULL
    AS_BAD_CAP,      // cap < 0, or cap > 0 with a NULL list
    AS_BAD_IDS,      // assign_at: m < 0, ids NULL with m > 0, an id outside [0, V)
};
inline const char *as_check_text(AsCheck c) {
    switch (c) {
    case AS_OK: return "ok";
    case AS_BAD_GROUPS: return "groups non-null, n_groups in [1, DPPR_ASSIGN_GROUPS_MAX]";
    case AS_BAD_SCALE: return "every scale finite and >= 0";
    case AS_BAD_MIN: return "min_score >= 0";
    case AS_BAD_DEST: return "dest 0 or 1";
    case AS_NULL_OUT: return "non-null out_label / out_counts";
    case AS_BAD_CAP: return "cap >= 0, and with cap > 0 non-null flip_id / flip_old / flip_new";
    case AS_BAD_IDS: return "m >= 0, ids in [0, V)";
    }
    return "?";
}

// scale: [C] (read only once the class table stands) -- every entry finite and >= 0 (false for NaN); NULL: fine
inline bool as_scale_ok(const double *scale, int C) {
    if (!scale) return true;
    for (int c = 0; c < C; ++c)
        if (!std::isfinite(scale[c]) || !(scale[c] >= 0.0)) return false;
    return true;
}
inline AsCheck as_common_check(const int32_t *groups, int32_t n_groups, double min_score) {
    if (!groups || n_groups < 1 || n_groups > AS_GROUPS_MAX) return AS_BAD_GROUPS;
    if (!(min_score >= 0.0)) return AS_BAD_MIN;
    return AS_OK;
}
inline AsCheck as_check(const int32_t *groups, int32_t n_groups, double min_score, int dest, const void *out_label, const void *out_counts,
                        int64_t cap, const void *flip_id, const void *flip_old, const void *flip_new) {
    if (const AsCheck c = as_common_check(groups, n_groups, min_score)) return c;
    if (dest != DPPR_DEST_HOST && dest != DPPR_DEST_DEVICE) return AS_BAD_DEST;
    if (!out_label || !out_counts) return AS_NULL_OUT;
    if (cap < 0 || (cap > 0 && (!flip_id || !flip_old || !flip_new))) return AS_BAD_CAP;
    return AS_OK;
}
inline AsCheck as_at_check(const int32_t *groups, int32_t n_groups, double min_score, const int32_t *ids, int32_t m, int64_t V,
                           const void *out_label) {
    if (const AsCheck c = as_common_check(groups, n_groups, min_score)) return c;
    if (!read_at_args_ok(ids, m, V)) return AS_BAD_IDS;
    if (!out_label) return AS_NULL_OUT;
    return AS_OK;
}

// the buffer of a point read (point_read of dppr_host_query.hpp, cols = 2, two outputs): a = (best, margin) per id, b = 16 bytes
// per id of which the first 8 are (label, second_label)
constexpr int AS_AT_COLS = 2;

} // namespace dppr
