// dppr_walk_plan.hpp -- the limits, the sizes, the range of a wave, the argument checks of the forward walks (dppr_walks,
// dppr_refine_at / dppr_group_refine_at) and THE definition of a walk: Philox4x32-10 and the step rule of include/dppr.h. Pure
// host code without HIP includes; the functions marked WALK_HD are also what the kernels of dppr_walk.hpp run, so the device and
// tests/native/walk_plan_test.cpp compile one and the same definition.
//
// A WALK is a function of (start external id v, walk number w, seed) and of the epoch's out-CSR alone. Step t = 0 .. 255 at
// internal vertex u:
//     (x0, x1, x2, x3) = philox(counter = (w, v, t, 0), key = (seed & 0xffffffff, seed >> 32))
//     x0 < WALK_STOP_BELOW                      -> the walk STOPS, endpoint = external id of u
//     d = out_row_ptr[u + 1] - out_row_ptr[u]     (0 for a start without an internal id)
//     j = floor((x1 * 2^32 + x2) * (d + 1) / 2^64)
//     j == d                                    -> the walk DIES, endpoint -1 (the `+ 1` of the reference's denominator)
//     else u = out_col[out_row_ptr[u] + j]
// and a walk alive after step 255 dies.
// INDEX SPACE of a call: walk (query q, number w) has index q * W + w, total = m * W <= 2^26; its endpoint goes to ends[index].
// A wave of the lane-refill kernel owns walk_range(total, wave): contiguous, whole multiples of 64 but for the last.
#pragma once

#include "dppr_query_plan.hpp"

#if defined(__HIPCC__)
#define WALK_HD __host__ __device__ __forceinline__
#else
#define WALK_HD inline
#endif

namespace dppr {

constexpr int64_t WALK_MAX_TOTAL = (int64_t)1 << 26; // walks of one call (the limits of m and W: include/dppr.h)

constexpr int WALK_MAX_STEPS = 256;
constexpr uint32_t WALK_STOP_BELOW = 0x26666666u; // floor(0.15 * 2^32)
constexpr int WALK_DIED = -1;                     // walk_step: the walk died
constexpr int WALK_STOPPED = -2;                  // walk_step: the walk stopped where it stands

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct Philox4 {
    uint32_t x0, x1, x2, x3;
};

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011)
WALK_HD Philox4 walk_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{c0, c1, c2, c3};
}

WALK_HD bool walk_stops(uint32_t x0) { return x0 < WALK_STOP_BELOW; }

// floor(((x1 * 2^32 + x2) * (d + 1)) / 2^64): 0 .. d, d the death slot
WALK_HD uint32_t walk_pick(uint32_t x1, uint32_t x2, uint32_t d) {
    const uint64_t x = ((uint64_t)x1 << 32) | x2, n = (uint64_t)d + 1;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__umul64hi(x, n);
#else
    return (uint32_t)(((unsigned __int128)x * n) >> 64);
#endif
}

// Step t of walk (v, w) at internal vertex u (u < 0: a start without an internal id, a row of no edges): the next vertex, or
// WALK_STOPPED / WALK_DIED. Two dependent loads on the way on: the row's bounds, then the column.
WALK_HD int walk_step(const int *row_ptr, const int *col, int u, uint32_t v, uint32_t w, uint32_t t, uint32_t k0, uint32_t k1) {
    const Philox4 x = walk_philox(w, v, t, 0u, k0, k1);
    if (walk_stops(x.x0)) return WALK_STOPPED;
    int rs = 0;
    uint32_t d = 0;
    if (u >= 0) {
        rs = row_ptr[u];
        d = (uint32_t)(row_ptr[u + 1] - rs);
    }
    const uint32_t j = walk_pick(x.x1, x.x2, d);
    if (j == d) return WALK_DIED;
    return col[(size_t)rs + j];
}

// The whole walk, restated plainly for the host: the endpoint's INTERNAL id, WALK_DIED, or -- for a walk that stopped on a start
// without an internal id -- WALK_STOPPED (its endpoint is v itself). *steps (may be null): draws taken.
inline int walk_run(const int *row_ptr, const int *col, int u0, uint32_t v, uint32_t w, uint64_t seed, int *steps = nullptr) {
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
    int u = u0;
    for (int t = 0; t < WALK_MAX_STEPS; ++t) {
        const int nx = walk_step(row_ptr, col, u, v, w, (uint32_t)t, k0, k1);
        if (steps) *steps = t + 1;
        if (nx == WALK_STOPPED) return u >= 0 ? u : WALK_STOPPED;
        if (nx == WALK_DIED) return WALK_DIED;
        u = nx;
    }
    return WALK_DIED;
}

// ---- sizes (64-bit throughout) and the index space ------------------------------------------------------------------------------
constexpr int64_t walk_total(int m, int W) { return (int64_t)m * (int64_t)W; }
constexpr size_t walk_ends_bytes(int m, int W) { return sizeof(int32_t) * (size_t)m * (size_t)W; }
constexpr size_t walk_result_elems(int m, int n) { return (size_t)3 * (size_t)m * (size_t)n; } // est | corr | sumsq, each [m][n]

constexpr int WALK_WAVE = 64;
constexpr int WALK_BLOCK = 256;                                  // threads of a workgroup: four waves
constexpr int WALK_WAVES_PER_BLOCK = WALK_BLOCK / WALK_WAVE;
constexpr int64_t WALK_TARGET_WAVES = 8192;                      // 256 CUs x 4 SIMDs x 8 waves: what the chip holds at once
constexpr int64_t WALK_RANGE_MAX = 1024;                         // walks of a wave's range at the most: 16 refills of every lane

// walks a wave owns: as many as spread the call over the chip's waves, whole multiples of 64, between 64 and WALK_RANGE_MAX
constexpr int64_t walk_per_wave(int64_t total) {
    int64_t per = (total + WALK_TARGET_WAVES - 1) / WALK_TARGET_WAVES;
    per = (per + WALK_WAVE - 1) / WALK_WAVE * WALK_WAVE;
    if (per < WALK_WAVE) per = WALK_WAVE;
    if (per > WALK_RANGE_MAX) per = WALK_RANGE_MAX;
    return per;
}
constexpr int64_t walk_waves(int64_t total) { return (total + walk_per_wave(total) - 1) / walk_per_wave(total); }
constexpr int64_t walk_blocks_refill(int64_t total) { return (walk_waves(total) + WALK_WAVES_PER_BLOCK - 1) / WALK_WAVES_PER_BLOCK; }
constexpr int64_t walk_blocks_simple(int64_t total) { return (total + WALK_BLOCK - 1) / WALK_BLOCK; }
// [lo, hi) of wave `wave` (empty for a wave beyond walk_waves)
WALK_HD void walk_range(int64_t total, int64_t per_wave, int64_t wave, int64_t *lo, int64_t *hi) {
    int64_t a = wave * per_wave, b = a + per_wave;
    if (a > total) a = total;
    if (b > total) b = total;
    *lo = a;
    *hi = b;
}

// ---- argument checks ------------------------------------------------------------------------------------------------------------
inline bool walk_sizes_ok(int64_t m, int64_t W) {
    return m >= 1 && m <= DPPR_WALK_MAX_M && W >= 1 && W <= DPPR_WALK_MAX_W && m * W <= WALK_MAX_TOTAL;
}
inline bool walk_dest_ok(int dest) { return dest == DPPR_DEST_HOST || dest == DPPR_DEST_DEVICE; }
inline bool walk_args_ok(const void *starts, int64_t m, int64_t W, int dest, const void *out_ends) {
    return walk_sizes_ok(m, W) && walk_dest_ok(dest) && starts && out_ends;
}
inline bool refine_args_ok(const void *ids, int64_t m, int64_t W, const void *out_est) { return walk_sizes_ok(m, W) && ids && out_est; }
// (the name tests/native/walk_plan_test.cpp checks it by)
inline bool walk_ids_ok(const int32_t *ids, int64_t m, int64_t V) { return ids_in_range(ids, m, V); }
// the state of a refine call: converged, and standing on the epoch the walks run over (-2: set by dppr_write, anything goes)
inline bool refine_epoch_ok(int last_epoch, int epoch_id) { return last_epoch == -2 || last_epoch == epoch_id; }

} // namespace dppr
