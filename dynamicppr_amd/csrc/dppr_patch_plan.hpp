// dppr_patch_plan.hpp -- the sizes, the result block and the argument checks of the patch feed (dppr_patch / dppr_group_patch).
// Pure host code without HIP includes (dppr_patch.hpp takes the tile and the head from it, dppr_host_query.hpp lays the workspace
// and the staging block out with it and checks a call with it; tests/native/patch_plan_test.cpp drives it on the CPU against a
// plain restatement).
//
// WORKSPACE, by the number of external ids V alone (every lane count fits):
//     mask  [V]               32 bits per external id: bit i = lane i is an UPSERT, bit 16 + i = lane i is a DELETE
//     cnt   [tiles][2][16]    int32: upserts, then deletes, of every lane in every tile of EX_TILE ids (2 n of the 32 in use)
//     base  [tiles][2][16]    int64: where the tile's first entry of a kind and lane goes (the lane's offset included)
// BLOCK of a patch: the head always, the sections only for a host destination (a device destination is written in place):
//     [up_offsets 17 x int64][del_offsets 17 x int64][go int32][written int32]  <- PT_HEAD_BYTES, always copied back
//     [up_ids cap_up x int32, padded to 8 bytes][up_p cap_up x double][del_ids cap_del x int32, padded to 8 bytes]
#pragma once

#include "dppr_export_plan.hpp"

namespace dppr {

constexpr int PT_LANES = Q_LANES;
constexpr size_t PT_HEAD_BYTES = 2 * 8 * (PT_LANES + 1) + 8;

struct PtHead {
    long long up_offsets[PT_LANES + 1];  // up_offsets[i] .. up_offsets[i + 1]: the upserts of source i; entries past n repeat [n]
    long long del_offsets[PT_LANES + 1]; // ... and its deletes
    int go;                              // 1: up_offsets[n] <= cap_up && del_offsets[n] <= cap_del, the fill and the re-mark ran
    int written;                         // what the call reports: go
};
static_assert(sizeof(PtHead) == PT_HEAD_BYTES, "the head of the block is twice 17 offsets, the go word and written");

struct PtWork {
    size_t mask_elems = 0; // uint32
    size_t cnt_elems = 0;  // int32
    size_t base_elems = 0; // int64
    size_t bytes = 0;
};

constexpr PtWork pt_workspace(int64_t V) {
    PtWork w;
    const size_t tiles = (size_t)(ex_tiles(V) > 0 ? ex_tiles(V) : 1);
    w.mask_elems = (size_t)(V > 0 ? V : 1);
    w.cnt_elems = tiles * 2 * PT_LANES;
    w.base_elems = tiles * 2 * PT_LANES;
    w.bytes = 4 * w.mask_elems + 4 * w.cnt_elems + 8 * w.base_elems;
    return w;
}

struct PtLayout {
    size_t off_up_ids = 0, off_up_p = 0, off_del_ids = 0;
    size_t total_bytes = 0; // head + sections: the device block, the pinned block and the one copy between them
};

// cap_up / cap_del entries of a HOST destination (caps of 0, and every device destination: the head alone)
constexpr PtLayout pt_layout(int64_t cap_up, int64_t cap_del) {
    PtLayout l;
    const size_t cu = (size_t)(cap_up > 0 ? cap_up : 0), cd = (size_t)(cap_del > 0 ? cap_del : 0);
    l.off_up_ids = PT_HEAD_BYTES;
    l.off_up_p = l.off_up_ids + pad8(sizeof(int32_t) * cu);
    l.off_del_ids = l.off_up_p + sizeof(double) * cu;
    l.total_bytes = l.off_del_ids + pad8(sizeof(int32_t) * cd);
    return l;
}

inline bool pt_remark_ok(int remark) {
    return remark == DPPR_PATCH_KEEP_MARK || remark == DPPR_PATCH_REMARK_ALL || remark == DPPR_PATCH_REMARK_EMITTED;
}

// the arguments of a patch that need no device: min_p >= 0 and min_delta >= 0 (false for NaN), caps >= 0, a known dest and remark,
// the out block with both offset arrays, and the arrays of a kind wherever one of its entries could be written
inline bool pt_args_ok(double min_p, double min_delta, int64_t cap_up, int64_t cap_del, int dest, int remark, const dppr_patch_out_t *out) {
    if (!(min_p >= 0.0) || !(min_delta >= 0.0) || cap_up < 0 || cap_del < 0) return false;
    if ((dest != DPPR_DEST_HOST && dest != DPPR_DEST_DEVICE) || !pt_remark_ok(remark)) return false;
    if (!out || !out->up_offsets || !out->del_offsets) return false;
    if (cap_up > 0 && !(out->up_ids && out->up_p)) return false;
    return cap_del == 0 || out->del_ids;
}

} // namespace dppr
