// walk_plan_test.cpp -- dynamicppr_amd/csrc/dppr_walk_plan.hpp on the CPU: the three Philox4x32-10 known answers, the stop
// threshold, the neighbour pick at its edges (d = 0, d = 2^31 - 2, x1:x2 = 0 and 2^64 - 1), the step rule and the whole walk on
// small graphs read through buffers of exactly the rows' sizes (the sanitizers watch the bounds), the ranges of the waves covering
// every index exactly once, 64-bit sizes, and the argument checks.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_walk_plan.hpp"

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

static void philox_known_answers() {
    struct Kat {
        uint32_t c[4], k[2], out[4];
    };
    const Kat kats[] = {
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
    };
    for (const Kat &k : kats) {
        const Philox4 x = walk_philox(k.c[0], k.c[1], k.c[2], k.c[3], k.k[0], k.k[1]);
        CHECK(x.x0 == k.out[0] && x.x1 == k.out[1] && x.x2 == k.out[2] && x.x3 == k.out[3], "%08x %08x %08x %08x", x.x0, x.x1, x.x2, x.x3);
    }
}

static void stop_and_pick() {
    CHECK(walk_stops(0u) && walk_stops(0x26666665u), "below the threshold");
    CHECK(!walk_stops(0x26666666u) && !walk_stops(0xffffffffu), "at and above the threshold");
    CHECK(WALK_STOP_BELOW == (uint32_t)(0.15 * 4294967296.0), "floor(0.15 * 2^32) = %u", (uint32_t)(0.15 * 4294967296.0));
    // d = 0: one choice, the death slot, whatever the draw
    CHECK(walk_pick(0u, 0u, 0u) == 0u && walk_pick(0xffffffffu, 0xffffffffu, 0u) == 0u && walk_pick(0x80000000u, 1u, 0u) == 0u, "d = 0");
    // d = 2^31 - 2: 2^31 - 1 choices; the smallest draw takes neighbour 0, the largest the death slot
    const uint32_t big = 0x7ffffffeu;
    CHECK(walk_pick(0u, 0u, big) == 0u, "x = 0");
    CHECK(walk_pick(0xffffffffu, 0xffffffffu, big) == big, "x = 2^64 - 1 gives %u", walk_pick(0xffffffffu, 0xffffffffu, big));
    CHECK(walk_pick(0xffffffffu, 0xffffffffu, 1u) == 1u && walk_pick(0x7fffffffu, 0xffffffffu, 1u) == 0u && walk_pick(0x80000000u, 0u, 1u) == 1u, "d = 1: halves");
    // every j in 0 .. d comes out, in order, as x grows (d = 6: seven equal slices)
    uint32_t last = 0;
    for (uint32_t k = 0; k < 7000; ++k) {
        const uint64_t x = (uint64_t)(((unsigned __int128)k << 64) / 7000);
        const uint32_t j = walk_pick((uint32_t)(x >> 32), (uint32_t)x, 6u);
        CHECK((j == k / 1000 || k % 1000 == 0) && j >= last && j <= 6u, "k %u j %u", k, j); // (at a slice's edge the floor of x decides)
        last = j;
    }
}

// the draw of step t of walk (v, w), for the tests that follow a walk by hand
static Philox4 draw(uint32_t v, uint32_t w, uint32_t t, uint64_t seed) {
    return walk_philox(w, v, t, 0u, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}

static void steps_and_walks() {
    // a graph of four vertices, rows exactly as long as their degrees: 0 -> {1, 1, 2}, 1 -> {}, 2 -> {0}, 3 -> {3}
    const std::vector<int> row_ptr = {0, 3, 3, 4, 5};
    const std::vector<int> col = {1, 1, 2, 0, 3};
    const uint64_t seeds[] = {0ull, 1ull, 0x9e3779b97f4a7c15ull};
    long stopped = 0, died = 0, total_steps = 0, n = 0;
    for (uint64_t seed : seeds)
        for (int u0 = -1; u0 < 4; ++u0)
            for (uint32_t w = 0; w < 400; ++w) {
                const uint32_t v = (uint32_t)(u0 + 10);
                // by hand
                int u = u0, want = WALK_DIED, want_steps = 0;
                for (int t = 0; t < WALK_MAX_STEPS; ++t) {
                    const Philox4 x = draw(v, w, (uint32_t)t, seed);
                    want_steps = t + 1;
                    if (x.x0 < 0x26666666u) {
                        want = u >= 0 ? u : WALK_STOPPED;
                        break;
                    }
                    const uint32_t d = u >= 0 ? (uint32_t)(row_ptr[(size_t)u + 1] - row_ptr[(size_t)u]) : 0u;
                    const uint64_t xx = ((uint64_t)x.x1 << 32) | x.x2;
                    const uint32_t j = (uint32_t)(((unsigned __int128)xx * (d + 1ull)) >> 64);
                    if (j == d) break;
                    u = col[(size_t)row_ptr[(size_t)u] + j];
                }
                int steps = 0;
                const int got = walk_run(row_ptr.data(), col.data(), u0, v, w, seed, &steps);
                CHECK(got == want && steps == want_steps, "seed %llx u0 %d w %u: %d (%d steps), want %d (%d)", (unsigned long long)seed, u0, w, got,
                      steps, want, want_steps);
                if (u0 == -1 || u0 == 1) CHECK(got == WALK_DIED || got == (u0 >= 0 ? u0 : WALK_STOPPED), "a start of degree 0 stops at itself or dies");
                if (u0 == 3) CHECK(got == WALK_DIED || got == 3, "a self-loop never leaves");
                stopped += got != WALK_DIED;
                died += got == WALK_DIED;
                total_steps += steps;
                ++n;
            }
    CHECK(stopped > n / 5 && died > n / 5, "both outcomes occur: %ld stopped, %ld died of %ld", stopped, died, n);
    CHECK(total_steps > n && total_steps < 8 * n, "%ld draws of %ld walks", total_steps, n);
    // a cycle that never dies by choice cannot be built (every vertex has its death slot); the truncation is reached only by
    // construction: walk_step is total for every t, and walk_run gives up after WALK_MAX_STEPS draws
    CHECK(WALK_MAX_STEPS == 256, "256 steps");
}

static void ranges() {
    const int64_t totals[] = {1, 63, 64, 65, 4097, 524288, 524289, (int64_t)1 << 20, ((int64_t)1 << 24) + 5, (int64_t)1 << 26};
    for (int64_t total : totals) {
        const int64_t per = walk_per_wave(total), waves = walk_waves(total);
        CHECK(per >= 64 && per <= WALK_RANGE_MAX && per % 64 == 0, "total %lld per %lld", (long long)total, (long long)per);
        CHECK(walk_blocks_refill(total) * WALK_WAVES_PER_BLOCK >= waves && (walk_blocks_refill(total) - 1) * WALK_WAVES_PER_BLOCK < waves, "blocks");
        CHECK(walk_blocks_simple(total) * WALK_BLOCK >= total && (walk_blocks_simple(total) - 1) * WALK_BLOCK < total, "blocks, simple");
        CHECK(walk_blocks_refill(total) < ((int64_t)1 << 31) && walk_blocks_simple(total) < ((int64_t)1 << 31), "a grid of 32 bits");
        int64_t expect = 0;
        bool ok = true;
        // every wave the grid starts, those beyond the last range included
        for (int64_t wv = 0; wv < walk_blocks_refill(total) * WALK_WAVES_PER_BLOCK; ++wv) {
            int64_t lo, hi;
            walk_range(total, per, wv, &lo, &hi);
            ok = ok && lo == expect && hi >= lo && hi - lo <= per && hi <= total && (wv < waves ? hi > lo : hi == lo);
            expect = hi;
        }
        CHECK(ok && expect == total, "total %lld: the ranges tile [0, total) in order", (long long)total);
    }
    CHECK(walk_per_wave(1) == 64 && walk_per_wave(524288) == 64 && walk_per_wave(524289) == 128 && walk_per_wave((int64_t)1 << 26) == 1024, "per wave");
    CHECK(walk_waves(1) == 1 && walk_waves(65) == 2 && walk_waves((int64_t)1 << 26) == 65536, "waves");
}

static void sizes_and_checks() {
    CHECK(walk_total(4096, 1 << 20) == ((int64_t)1 << 32), "64-bit product");
    CHECK(walk_ends_bytes(4096, 16384) == ((size_t)1 << 28), "bytes of the largest call");
    CHECK(walk_result_elems(4096, 16) == (size_t)3 * 65536, "results");
    int x = 0;
    const void *p = &x;
    CHECK(walk_sizes_ok(1, 1) && walk_sizes_ok(4096, 16384) && walk_sizes_ok(64, 1 << 20) && walk_sizes_ok(1, 1 << 20), "limits, inside");
    CHECK(!walk_sizes_ok(0, 1) && !walk_sizes_ok(1, 0) && !walk_sizes_ok(-1, 5) && !walk_sizes_ok(5, -1), "below");
    CHECK(!walk_sizes_ok(4097, 1) && !walk_sizes_ok(1, (1 << 20) + 1) && !walk_sizes_ok(65, 1 << 20) && !walk_sizes_ok(4096, 16385), "above");
    CHECK(walk_args_ok(p, 1, 1, 0, p) && walk_args_ok(p, 1, 1, 1, p), "walks");
    CHECK(!walk_args_ok(nullptr, 1, 1, 0, p) && !walk_args_ok(p, 1, 1, 0, nullptr) && !walk_args_ok(p, 1, 1, 2, p) && !walk_args_ok(p, 1, 1, -1, p) &&
              !walk_args_ok(p, 0, 1, 0, p),
          "walks, rejected");
    CHECK(refine_args_ok(p, 3, 7, p) && !refine_args_ok(nullptr, 3, 7, p) && !refine_args_ok(p, 3, 7, nullptr) && !refine_args_ok(p, 3, 0, p), "refine");
    const int32_t ids[4] = {0, 9, 3, 9};
    CHECK(walk_ids_ok(ids, 4, 10) && !walk_ids_ok(ids, 4, 9) && walk_ids_ok(ids, 0, 0), "ids");
    const int32_t neg[2] = {1, -1};
    CHECK(!walk_ids_ok(neg, 2, 10) && walk_ids_ok(neg, 1, 10), "a negative id");
    CHECK(refine_epoch_ok(-2, 7) && refine_epoch_ok(7, 7) && !refine_epoch_ok(6, 7) && !refine_epoch_ok(-1, 0), "epochs");
}

int main() {
    philox_known_answers();
    stop_and_pick();
    steps_and_walks();
    ranges();
    sizes_and_checks();
    std::printf("walk_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
