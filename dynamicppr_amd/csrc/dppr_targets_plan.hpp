// dppr_targets_plan.hpp -- weighted vertex sets as the targets of a source group (dppr_add_target_group /
// dppr_group_replace_target / dppr_group_targets): the argument check, the host mirror of a group's seed sets (external ids
// ascending within a lane), the device table built from it through an ext -> int lookup (internal ids ascending within a lane:
// the stream update finds a tail's weight by binary search), the table under a renumbering's permutation, what replace / add /
// remove do to the lanes, and the dppr_group_sources projection. Pure host code without HIP includes (dppr_engine.hip plans with
// it and launches dppr_targets.hpp; tests/native/targets_plan_test.cpp drives it on the CPU under the sanitizers).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace dppr {

constexpr int TG_LANES = 16;               // lanes of a group (GS_MAX of dppr_multi.hpp, asserted equal in dppr_engine.hip)
constexpr int64_t TG_SET_MAX = 65536;      // seeds of one lane (DPPR_TARGET_SET_MAX of include/dppr.h, asserted equal in dppr_engine.hip)

enum TgCheck { TG_OK = 0, TG_BAD_N, TG_NULL, TG_BAD_OFFSETS, TG_BAD_SIZE, TG_BAD_ID, TG_DUP_ID, TG_BAD_WEIGHT };

inline const char *tg_check_text(TgCheck c) {
    switch (c) {
    case TG_OK: return "ok";
    case TG_BAD_N: return "1..16 lanes";
    case TG_NULL: return "NULL offsets, ids or weights";
    case TG_BAD_OFFSETS: return "offsets start at 0 and never decrease";
    case TG_BAD_SIZE: return "a lane holds 1..DPPR_TARGET_SET_MAX seeds";
    case TG_BAD_ID: return "vertex out of range";
    case TG_DUP_ID: return "a vertex twice in one lane";
    default: return "weights are finite and > 0";
    }
}

// one lane: m seeds, ids in [0, V), none twice, every weight finite and > 0 (reads exactly m entries of each array)
inline TgCheck tg_check_lane(const int32_t *ids, const double *weights, int64_t m, int64_t V) {
    if (m < 1 || m > TG_SET_MAX) return TG_BAD_SIZE;
    if (!ids || !weights) return TG_NULL;
    for (int64_t i = 0; i < m; ++i)
        if (ids[i] < 0 || ids[i] >= V) return TG_BAD_ID;
    for (int64_t i = 0; i < m; ++i)
        if (!(weights[i] > 0.0) || !std::isfinite(weights[i])) return TG_BAD_WEIGHT;
    std::vector<int32_t> s(ids, ids + m);
    std::sort(s.begin(), s.end());
    return std::adjacent_find(s.begin(), s.end()) != s.end() ? TG_DUP_ID : TG_OK;
}

// a whole group: offsets [n + 1], lane i = [offsets[i], offsets[i + 1]). The offsets are checked before any id is read.
inline TgCheck tg_check(const int64_t *offsets, const int32_t *ids, const double *weights, int64_t n, int64_t V) {
    if (n < 1 || n > TG_LANES) return TG_BAD_N;
    if (!offsets || !ids || !weights) return TG_NULL;
    if (offsets[0] != 0) return TG_BAD_OFFSETS;
    for (int64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return TG_BAD_OFFSETS;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t m = offsets[i + 1] - offsets[i];
        if (m < 1 || m > TG_SET_MAX) return TG_BAD_SIZE;
    }
    for (int64_t i = 0; i < n; ++i)
        if (TgCheck c = tg_check_lane(ids + offsets[i], weights + offsets[i], offsets[i + 1] - offsets[i], V)) return c;
    return TG_OK;
}

struct TgSeed {
    int32_t id; // external id in TargetSets, internal id in a lane being built for the table
    double w;
};

// The host mirror of a group's seed sets. n == 0: the group has none (every lane is a plain source and the group runs the
// code of dppr_add_source_group).
struct TargetSets {
    int n = 0;
    std::vector<TgSeed> lane[TG_LANES]; // external ids ascending

    int64_t total() const {
        int64_t t = 0;
        for (int i = 0; i < n; ++i) t += (int64_t)lane[i].size();
        return t;
    }
};

inline std::vector<TgSeed> tg_lane(const int32_t *ids, const double *weights, int64_t m) {
    std::vector<TgSeed> l((size_t)m);
    for (int64_t i = 0; i < m; ++i) l[(size_t)i] = {ids[i], weights[i]};
    std::sort(l.begin(), l.end(), [](const TgSeed &a, const TgSeed &b) { return a.id < b.id; });
    return l;
}
inline std::vector<TgSeed> tg_source_lane(int32_t source) { return {TgSeed{source, 1.0}}; }

// (arguments that passed tg_check)
inline TargetSets tg_build(const int64_t *offsets, const int32_t *ids, const double *weights, int n) {
    TargetSets ts;
    ts.n = n;
    for (int i = 0; i < n; ++i) ts.lane[i] = tg_lane(ids + offsets[i], weights + offsets[i], offsets[i + 1] - offsets[i]);
    return ts;
}

// A lane of one seed of weight exactly 1.0 IS a source lane: Init gives it r = e_s, as gpu/PPRCommon.cuh:12-22 does.
inline bool tg_is_source(const std::vector<TgSeed> &l) { return l.size() == 1 && l[0].w == 1.0; }
inline bool tg_has_set(const TargetSets &ts) {
    for (int i = 0; i < ts.n; ++i)
        if (!tg_is_source(ts.lane[i])) return true;
    return false;
}
// what dppr_group_sources reports: the vertex of a source lane, -1 for a set lane
inline void tg_sources(const TargetSets &ts, int32_t *out /* [ts.n] */) {
    for (int i = 0; i < ts.n; ++i) out[i] = tg_is_source(ts.lane[i]) ? ts.lane[i][0].id : -1;
}

// Lanes after a change of the group (dppr_churn_plan.hpp: new lane j takes old lane map[j], -1: nothing yet); the lane that
// is (re)initialised receives `fresh`.
inline TargetSets tg_relane(const TargetSets &ts, const int *map /* [TG_LANES] */, int n_new, int fresh_lane, std::vector<TgSeed> fresh) {
    TargetSets out;
    out.n = n_new;
    for (int j = 0; j < n_new; ++j)
        if (map[j] >= 0 && map[j] < ts.n) out.lane[j] = ts.lane[map[j]];
    if (fresh_lane >= 0 && fresh_lane < n_new) out.lane[fresh_lane] = std::move(fresh);
    return out;
}

// The device table: one block of bytes, weights first (8-byte aligned), then the 17 lane offsets, then the ids.
//   w   [total]  double   at tg_w_at()
//   off [17]     int      at tg_off_at(total)    (lanes beyond n: empty, off[i] = total)
//   ids [total]  int      at tg_ids_at(total)    internal ids, ascending within a lane
struct TgTable {
    int off[TG_LANES + 1] = {0};
    std::vector<int32_t> ids;
    std::vector<double> w;
    int total() const { return off[TG_LANES]; }
};
constexpr size_t tg_w_at() { return 0; }
constexpr size_t tg_off_at(int64_t total) { return sizeof(double) * (size_t)total; }
constexpr size_t tg_ids_at(int64_t total) { return tg_off_at(total) + sizeof(int) * (TG_LANES + 1); }
constexpr size_t tg_bytes(int64_t total) { return (tg_ids_at(total) + sizeof(int) * (size_t)total + 7) & ~(size_t)7; }

inline void tg_sort_lanes(TgTable &t) {
    std::vector<std::pair<int32_t, double>> l;
    for (int i = 0; i < TG_LANES; ++i) {
        const int a = t.off[i], b = t.off[i + 1];
        l.clear();
        for (int k = a; k < b; ++k) l.emplace_back(t.ids[(size_t)k], t.w[(size_t)k]);
        std::sort(l.begin(), l.end(), [](const std::pair<int32_t, double> &x, const std::pair<int32_t, double> &y) { return x.first < y.first; });
        for (int k = a; k < b; ++k) {
            t.ids[(size_t)k] = l[(size_t)(k - a)].first;
            t.w[(size_t)k] = l[(size_t)(k - a)].second;
        }
    }
}

// ext2int(external id) -> internal id (every seed has one: the engine assigns them before it builds a table)
template <class Ext2Int>
inline TgTable tg_table(const TargetSets &ts, Ext2Int ext2int) {
    TgTable t;
    const int64_t total = ts.total();
    t.ids.reserve((size_t)total);
    t.w.reserve((size_t)total);
    for (int i = 0; i < TG_LANES; ++i) {
        if (i < ts.n)
            for (const TgSeed &s : ts.lane[i]) {
                t.ids.push_back((int32_t)ext2int(s.id));
                t.w.push_back(s.w);
            }
        t.off[i + 1] = (int)t.ids.size();
    }
    tg_sort_lanes(t);
    return t;
}

// a renumbering: perm[old internal id] = new internal id; the lanes are sorted again
inline void tg_remap(TgTable &t, const int32_t *perm) {
    for (auto &v : t.ids) v = perm[(size_t)v];
    tg_sort_lanes(t);
}

// the block the device reads (tg_bytes(total) bytes)
inline void tg_pack(const TgTable &t, unsigned char *blob) {
    const int total = t.total();
    double *w = reinterpret_cast<double *>(blob + tg_w_at());
    int *off = reinterpret_cast<int *>(blob + tg_off_at(total));
    int *ids = reinterpret_cast<int *>(blob + tg_ids_at(total));
    for (int k = 0; k < total; ++k) w[k] = t.w[(size_t)k];
    for (int i = 0; i <= TG_LANES; ++i) off[i] = t.off[i];
    for (int k = 0; k < total; ++k) ids[k] = t.ids[(size_t)k];
}

// h of a lane at an internal id, as the device looks it up: binary search in the lane's slice, 0.0 when it is no seed
inline double tg_weight_at(const TgTable &t, int lane, int32_t v) {
    int lo = t.off[lane], hi = t.off[lane + 1];
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (t.ids[(size_t)mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo < t.off[lane + 1] && t.ids[(size_t)lo] == v ? t.w[(size_t)lo] : 0.0;
}

// dppr_group_targets: the TRUE offsets always; ids and weights (external ids ascending within a lane) only when cap suffices
inline void tg_list(const TargetSets &ts, int64_t *out_offsets /* [TG_LANES + 1] */, int32_t *out_ids, double *out_weights, int64_t cap) {
    int64_t at = 0;
    out_offsets[0] = 0;
    for (int i = 0; i < TG_LANES; ++i) {
        if (i < ts.n) at += (int64_t)ts.lane[i].size();
        out_offsets[i + 1] = at;
    }
    if (at > cap || !out_ids || !out_weights) return;
    int64_t k = 0;
    for (int i = 0; i < ts.n; ++i)
        for (const TgSeed &s : ts.lane[i]) {
            out_ids[k] = s.id;
            out_weights[k] = s.w;
            ++k;
        }
}

} // namespace dppr
