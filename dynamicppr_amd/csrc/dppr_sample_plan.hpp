// dppr_sample_plan.hpp -- what the sampling queries (dppr_sample / dppr_group_sample) decide before any device is involved: the
// limits and the check of a call's arguments, the SHAPE of the sum tree of a lane -- the tiles, the stored levels and where each
// of them lies in the node array --, the sizes of the workspace and the layout of the result block; and THE definition of a draw
// of include/dppr.h: the uniform, the scaling and the step of the descent. Pure host code without HIP includes; the functions
// marked WALK_HD are also what the kernels of dppr_sample.hpp run (as dppr_walk_plan.hpp shares walk_philox, which is the Philox
// of a draw too), so the device and tests/native/sample_plan_test.cpp compile one and the same definition.
//
// TREE. The leaves of a lane are its weights in EXTERNAL id order, padded with +0.0 to Vt = V rounded up to SM_TILE = 2048; a
// TILE is 2048 leaves, a SUBTILE 256. Level l + 1 is y[j] = y_l[2j] + y_l[2j + 1]. x + (+0.0) == x and (+0.0) + (+0.0) == +0.0,
// so padding a level with +0.0 nodes changes no value above it: the tree over P leaves (P the smallest power of two >= V) of
// include/dppr.h and the tree over Vt leaves agree in every node both have, a node that only one of them has is +0.0, and where
// P < 2048 the levels between log2(P) and 11 repeat the root with a +0.0 sibling, which the descent never enters. So every lane
// has the levels 0 .. top, top = 11 + ceil(log2(tiles)): level l <= 11 holds Vt >> l nodes, level l > 11 holds
// ceil(tiles / 2^(l - 11)); the root is the one node of level `top`. A child beyond the count of its level is +0.0.
// STORED: the leaves [n][Vt], lane-major (a subtile of a lane is 2 KB contiguous), and the levels 8 .. top in the node array
// [n][node_stride], level l at off[l]. Levels 1 .. 7 are rebuilt by the draw from the 256 leaves of a subtile; only
// dppr_debug_sample_form(1) stores them too, in a third array [n][Vt] with level l at sample_low_off(Vt, l).
// BLOCK, one copy to the host: [16 totals] [16 supports] [16 statuses] <- SM_HEAD_BYTES = 256, then -- a host destination --
// ids [n][S] int32 and, 8-aligned, w [n][S] doubles.
#pragma once

#include "dppr_rank_plan.hpp"
#include "dppr_walk_plan.hpp"

namespace dppr {

constexpr int SM_TILE = 2048;      // leaves of a tile: one workgroup of k_sm_leaves
constexpr int SM_SUB = 256;        // leaves of a subtile: what a wave of k_sm_draw rebuilds, four per lane
constexpr int SM_SUB_LEVEL = 8;    // the first stored level: one node per subtile
constexpr int SM_TILE_LEVEL = 11;  // one node per tile
constexpr int SM_BLOCK = 256;      // threads of every kernel of dppr_sample.hpp: four waves
constexpr int SM_MAX_LEVELS = 32;  // levels 0 .. 31: V < 2^31
constexpr uint32_t SM_DOMAIN = 0x53414D50u; // "SAMP": the fourth counter word of a draw
static_assert(SM_TILE == 1 << SM_TILE_LEVEL && SM_SUB == 1 << SM_SUB_LEVEL, "levels and sizes name the same thing");

// ---- THE definition of a draw ---------------------------------------------------------------------------------------------------
// u = ((x0 * 2^32 + x1) >> 11) * 2^-53: 53 bits, exact, in [0, 1)
WALK_HD double sample_uniform(uint32_t x0, uint32_t x1) {
    const uint64_t m = (((uint64_t)x0 << 32) | (uint64_t)x1) >> 11;
    return (double)m * 0x1p-53;
}
// the uniform of draw number j of lane i
WALK_HD double sample_u(uint64_t j, uint32_t lane, uint64_t seed) {
    const Philox4 r = walk_philox((uint32_t)(j & 0xffffffffu), (uint32_t)(j >> 32), lane, SM_DOMAIN, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
    return sample_uniform(r.x0, r.x1);
}
// x = u * root, one rounding
WALK_HD double sample_scale(double u, double root) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(u, root);
#else
    return u * root;
#endif
}
// One step of the descent at a node with children L (even) and R (odd): true = go right, with x = x - L (one rounding).
WALK_HD bool sample_step(double &x, double L, double R) {
    if (x >= L && R > 0.0) {
#if defined(__HIP_DEVICE_COMPILE__)
        x = __dsub_rn(x, L);
#else
        x = x - L;
#endif
        return true;
    }
    return false;
}
// the weight of a score
WALK_HD double sample_weight(double score, double min_score) { return score > min_score ? score : 0.0; }
// the status of a root
WALK_HD int sample_status(double root) {
    if (root == 0.0) return DPPR_SAMPLE_EMPTY;
    if (!(root - root == 0.0)) return DPPR_SAMPLE_NONFINITE; // (inf - inf and NaN - NaN are NaN)
    return DPPR_SAMPLE_OK;
}

// ... restated plainly for the host: the tree of include/dppr.h over P leaves, level by level
inline int64_t sample_pow2(int64_t V) {
    int64_t P = 1;
    while (P < V) P <<= 1;
    return P;
}
inline void sample_tree_ref(const double *w, int64_t V, std::vector<std::vector<double>> &levels) {
    const int64_t P = sample_pow2(V);
    levels.clear();
    levels.emplace_back((size_t)P, 0.0);
    for (int64_t j = 0; j < V; ++j) levels[0][(size_t)j] = w[j];
    while (levels.back().size() > 1) {
        const std::vector<double> &lo = levels.back();
        std::vector<double> up(lo.size() / 2);
        for (size_t j = 0; j < up.size(); ++j) up[j] = lo[2 * j] + lo[2 * j + 1];
        levels.push_back(std::move(up));
    }
}
// the leaf of x (= u * root) in a tree with a finite root > 0
inline int64_t sample_descend_ref(const std::vector<std::vector<double>> &levels, double x) {
    int64_t k = 0;
    for (size_t l = levels.size() - 1; l > 0; --l) {
        const double L = levels[l - 1][(size_t)(2 * k)], R = levels[l - 1][(size_t)(2 * k + 1)];
        k = 2 * k + (sample_step(x, L, R) ? 1 : 0);
    }
    return k;
}
// draw number j of lane i: the external id, -1 where the root is zero or not finite
inline int64_t sample_draw_ref(const std::vector<std::vector<double>> &levels, uint64_t j, uint32_t lane, uint64_t seed) {
    const double root = levels.back()[0];
    if (sample_status(root) != DPPR_SAMPLE_OK) return -1;
    return sample_descend_ref(levels, sample_scale(sample_u(j, lane, seed), root));
}

// ---- the shape of a lane's stored tree --------------------------------------------------------------------------------------------
struct SmTree {
    int top = SM_TILE_LEVEL;         // the level of the root
    int tiles = 1;
    long long Vt = SM_TILE;          // padded leaves of a lane
    unsigned cnt[SM_MAX_LEVELS] = {0}; // nodes of level l (l >= SM_SUB_LEVEL; 0 below and above top)
    unsigned off[SM_MAX_LEVELS] = {0}; // ... and where they start in a lane's node array
    unsigned node_stride = 0;        // doubles of a lane's node array (even)
};
inline SmTree sample_tree(int64_t V) {
    SmTree t;
    t.tiles = (int)((V + SM_TILE - 1) / SM_TILE);
    if (t.tiles < 1) t.tiles = 1;
    t.Vt = (long long)t.tiles * SM_TILE;
    unsigned at = 0;
    for (int l = SM_SUB_LEVEL; l < SM_MAX_LEVELS; ++l) {
        const unsigned c = l <= SM_TILE_LEVEL ? (unsigned)(t.Vt >> l) : (t.cnt[l - 1] + 1) / 2;
        t.cnt[l] = c;
        t.off[l] = at;
        at += (c + 1) & ~1u; // (every level starts on 16 bytes)
        t.top = l;
        if (l >= SM_TILE_LEVEL && c == 1) break;
    }
    t.node_stride = at;
    return t;
}
// where level l (1 .. 7) of a lane lies in the array of the low levels (dppr_debug_sample_form(1)): Vt >> l nodes each
constexpr long long sample_low_off(long long Vt, int l) { return Vt - (Vt >> (l - 1)); }

// ---- sizes (64-bit throughout) ------------------------------------------------------------------------------------------------------
constexpr size_t sample_leaf_elems(int n, long long Vt) { return (size_t)n * (size_t)Vt; }
inline size_t sample_node_elems(int n, const SmTree &t) { return (size_t)n * (size_t)t.node_stride; }
// the workspace of a call without the block, in bytes: 8 n Vt (1 + 1/128) and a few doubles per level
inline size_t sample_work_bytes(int n, int64_t V) {
    const SmTree t = sample_tree(V);
    return sizeof(double) * (sample_leaf_elems(n, t.Vt) + sample_node_elems(n, t));
}

constexpr size_t SM_HEAD_BYTES = 256;
struct SmLayout {
    size_t off_total = 0, off_support = 128, off_status = 192, off_ids = SM_HEAD_BYTES, off_w = SM_HEAD_BYTES;
    size_t total_bytes = SM_HEAD_BYTES;
};
constexpr SmLayout sample_layout(int n, int64_t S, bool host, bool with_w) {
    SmLayout l;
    if (!host) return l;
    const size_t ns = (size_t)n * (size_t)S;
    l.off_w = (l.off_ids + sizeof(int32_t) * ns + 7) & ~(size_t)7;
    l.total_bytes = l.off_w + (with_w ? sizeof(double) * ns : 0);
    return l;
}
constexpr size_t sample_ids_bytes(int n, int64_t S) { return sizeof(int32_t) * (size_t)n * (size_t)S; }
constexpr size_t sample_w_bytes(int n, int64_t S) { return sizeof(double) * (size_t)n * (size_t)S; }

// draws of one call: index t = i * S + (j - first); a wave of k_sm_draw owns a contiguous range of them, 64 at a time
constexpr int64_t SM_DRAWS_PER_WAVE = 256;
constexpr int64_t sample_draw_blocks(int64_t total) {
    return (total + SM_DRAWS_PER_WAVE * (SM_BLOCK / 64) - 1) / (SM_DRAWS_PER_WAVE * (SM_BLOCK / 64));
}
constexpr int64_t sample_plain_blocks(int64_t total) { return (total + SM_BLOCK - 1) / SM_BLOCK; }

// ---- argument checks ------------------------------------------------------------------------------------------------------------------
inline bool sample_sizes_ok(int64_t n, int64_t S) {
    return n >= 1 && n <= Q_LANES && S >= 0 && S <= DPPR_SAMPLE_MAX && n * S <= DPPR_SAMPLE_MAX_TOTAL;
}
inline bool sample_first_ok(uint64_t first, int64_t S) { return S >= 0 && first + (uint64_t)S >= first; } // first + S does not wrap
inline bool sample_dest_ok(int dest) { return dest == DPPR_DEST_HOST || dest == DPPR_DEST_DEVICE; }
inline bool sample_min_ok(double min_score) { return min_score >= 0.0; } // (false for a NaN)
inline bool sample_form_ok(int form) { return form == 0 || form == 1; }
inline bool sample_args_ok(const dppr_rank_spec_t *s, double min_score, int64_t n, uint64_t first, int64_t S, int dest, const void *out_ids,
                           const void *out_total, const void *out_status) {
    if (!rank_spec_ok(s) || !sample_min_ok(min_score) || !sample_sizes_ok(n, S) || !sample_first_ok(first, S) || !sample_dest_ok(dest)) return false;
    if (S > 0 && !out_ids) return false;
    return out_total && out_status;
}

} // namespace dppr
