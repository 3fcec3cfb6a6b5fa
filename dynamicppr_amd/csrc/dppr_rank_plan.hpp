// dppr_rank_plan.hpp -- what the ranked queries (dppr_topk_ranked / dppr_group_topk_ranked / dppr_rank_score_at /
// dppr_group_rank_score_at) decide before any device is involved: the check of a spec and of a call's arguments, whether a spec
// needs the epoch's CSRs at all, the seeds of a call's lanes as one flat list, the PIECE LIST of the marking stage -- the rows of
// the seeds cut into pieces of at most `piece` entries, one wave of k_rk_mark each -- with the bound on its length, and the sizes
// of the stage's buffers. Pure host code without HIP includes (dppr_host_query.hpp checks a call and plans its marking stage with it;
// tests/native/rank_plan_test.cpp drives it on the CPU under the sanitizers).
//
// A piece is an item of the conductance sweep's chunk list (dppr_cluster_plan.hpp: cl_item): position | direction | chunk number.
// The position is the index of a seed in the call's flat seed list (lane 0's seeds, then lane 1's, ..), the direction 0 the seed's
// out-row (DPPR_EXCLUDE_OUT_NEIGHBOURS) and 1 its in-row (DPPR_EXCLUDE_IN_NEIGHBOURS).
#pragma once

#include <vector>

#include "dppr_cluster_plan.hpp"

namespace dppr {

constexpr int RK_PIECE = 512;   // entries of a row one wave of k_rk_mark walks (dppr_debug_rank_piece lowers it)
constexpr int RK_BLOCK = 256;   // the kernels of dppr_rank.hpp but k_rk_scores (the tile of dppr_topk.hpp): four waves
constexpr int RK_WAVES = RK_BLOCK / 64;
constexpr uint32_t RK_EXCLUDE_ALL = DPPR_EXCLUDE_SEEDS | DPPR_EXCLUDE_IN_NEIGHBOURS | DPPR_EXCLUDE_OUT_NEIGHBOURS;
constexpr uint32_t RK_EXCLUDE_ROWS = DPPR_EXCLUDE_IN_NEIGHBOURS | DPPR_EXCLUDE_OUT_NEIGHBOURS; // the flags that walk a row

inline bool rank_piece_ok(int edges) { return edges >= 1 && edges <= RK_PIECE; }

// a spec as the kernels read it: NULL is the spec of all zeros
struct RkSpec {
    int factor = DPPR_FACTOR_NONE, factor_dtype = DPPR_F64, mask = DPPR_MASK_NONE;
    const void *factor_dev = nullptr;
    const uint8_t *mask_dev = nullptr;
    uint32_t exclude = 0;
};
inline RkSpec rank_spec(const dppr_rank_spec_t *s) {
    RkSpec r;
    if (!s) return r;
    r.factor = s->factor;
    r.factor_dtype = s->factor_dtype;
    r.factor_dev = s->factor == DPPR_FACTOR_DEV ? s->factor_dev : nullptr;
    r.mask = s->mask;
    r.mask_dev = s->mask != DPPR_MASK_NONE ? s->mask_dev : nullptr;
    r.exclude = s->exclude;
    return r;
}

// every enum value known, no unknown exclude bit (the dtype is read only for DPPR_FACTOR_DEV)
inline bool rank_spec_ok(const dppr_rank_spec_t *s) {
    if (!s) return true;
    if (s->factor < DPPR_FACTOR_NONE || s->factor > DPPR_FACTOR_INV_DEG) return false;
    if (s->factor == DPPR_FACTOR_DEV && s->factor_dtype != DPPR_F64 && s->factor_dtype != DPPR_F32) return false;
    if (s->mask < DPPR_MASK_NONE || s->mask > DPPR_MASK_DENY) return false;
    return (s->exclude & ~RK_EXCLUDE_ALL) == 0;
}
// does the spec read the epoch's CSRs (degrees or neighbours)? Without, `epoch` is not looked at.
inline bool rank_needs_epoch(const dppr_rank_spec_t *s) {
    return s && (s->factor == DPPR_FACTOR_DEG || s->factor == DPPR_FACTOR_INV_DEG || (s->exclude & RK_EXCLUDE_ROWS) != 0);
}
inline bool rank_needs_factor_dev(const dppr_rank_spec_t *s) { return s && s->factor == DPPR_FACTOR_DEV; }
inline bool rank_needs_mask_dev(const dppr_rank_spec_t *s) { return s && s->mask != DPPR_MASK_NONE; }
constexpr size_t rank_factor_elem_bytes(int dtype) { return dtype == DPPR_F32 ? sizeof(float) : sizeof(double); }
constexpr size_t rank_factor_bytes(int dtype, int64_t V) { return rank_factor_elem_bytes(dtype) * (size_t)V; }
constexpr size_t rank_mask_bytes(int64_t V) { return (size_t)V; }

inline bool rank_topk_args_ok(const dppr_rank_spec_t *s, int32_t k, double min_score, const void *ids, const void *score, const void *cnt) {
    return rank_spec_ok(s) && topk_args_ok(k, min_score, ids, score, cnt);
}
inline bool rank_score_at_args_ok(const dppr_rank_spec_t *s, const int32_t *ids, int32_t m, int64_t V, const void *out) {
    return rank_spec_ok(s) && out && read_at_args_ok(ids, m, V);
}

// The seeds of a call's lanes as one flat list: lane i holds positions [off[i], off[i + 1]). A source lane (src[i] >= 0) has one
// seed; a set lane has the tg_off[i + 1] - tg_off[i] seeds of the group's seed table (tg_off NULL: the group has no table).
struct RkSeeds {
    int n = 0;
    int off[Q_LANES + 1] = {0};
    int total() const { return off[Q_LANES]; }
};
inline RkSeeds rk_seeds(const int *src /* [n] */, const int *tg_off /* [17] or NULL */, int n) {
    RkSeeds s;
    s.n = n;
    for (int i = 0; i < Q_LANES; ++i) {
        int cnt = 0;
        if (i < n) cnt = src[i] >= 0 ? 1 : tg_off ? tg_off[i + 1] - tg_off[i] : 0;
        s.off[i + 1] = s.off[i] + cnt;
    }
    return s;
}
// the lane that holds position pos (pos < total)
inline int rk_lane_of(const RkSeeds &s, int pos) {
    int lane = 0;
    while (lane + 1 < Q_LANES && pos >= s.off[lane + 1]) ++lane;
    return lane;
}

constexpr long long rk_chunks(long long len, int piece) { return (len + piece - 1) / piece; }

// The piece list of a call. len [total][2]: the out-row and the in-row length of every seed, in list order. A row of length 0
// has no piece; rows are walked only in the directions `exclude` names. Items are in position order, out-row before in-row,
// chunks ascending (the order is no part of the result: k_rk_mark only ORs bits).
inline void rk_pieces(const int *len, int total, uint32_t exclude, int piece, std::vector<unsigned long long> &out) {
    out.clear();
    for (int pos = 0; pos < total; ++pos)
        for (unsigned dir = 0; dir < 2; ++dir) {
            if (!(exclude & (dir ? DPPR_EXCLUDE_IN_NEIGHBOURS : DPPR_EXCLUDE_OUT_NEIGHBOURS))) continue;
            const long long chunks = rk_chunks(len[2 * (size_t)pos + dir], piece);
            for (long long c = 0; c < chunks; ++c) out.push_back(cl_item((unsigned)pos, dir, (unsigned)c));
        }
}
// Pieces a call can have, known before any row length is: the seeds of a lane are distinct vertices, so their rows of one direction
// hold at most Ed entries together, and a row of len > 0 entries has at most len / piece + 1 pieces.
inline size_t rk_piece_cap(const RkSeeds &s, long long Ed, uint32_t exclude, int piece) {
    const size_t dirs = ((exclude & DPPR_EXCLUDE_IN_NEIGHBOURS) ? 1 : 0) + ((exclude & DPPR_EXCLUDE_OUT_NEIGHBOURS) ? 1 : 0);
    return dirs * ((size_t)s.total() + (size_t)s.n * (size_t)(Ed / piece + 1));
}

// the marking stage's buffers: the exclusion word of every live row, the two row lengths of every seed (the scratch state is sized
// by dppr_query_plan.hpp)
constexpr size_t rk_excl_elems(size_t n_int) { return n_int > 0 ? n_int : 1; }
constexpr size_t rk_len_elems(size_t total_seeds) { return 2 * (total_seeds > 0 ? total_seeds : 1); }

} // namespace dppr
