// sample_plan_test.cpp -- dynamicppr_amd/csrc/dppr_sample_plan.hpp on the CPU: the stored levels of a lane's tree (counts, offsets
// that do not overlap and are aligned, the root's level against the definition's log2(P)), the result block, every rejection of a
// call's arguments at its limit, the uniform at both ends, the descent against a brute-force linear scan on exact dyadic weights,
// the shared step never entering a zero node over random trees with zeros, and the stored shape -- tiles, missing nodes as +0.0,
// the levels above the root of a small tree -- giving the tree of the definition.
// Every array is exactly as long as the code may touch (the sanitizers watch the bounds).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_sample_plan.hpp"

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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void shapes() {
    const int64_t Vs[] = {1, 2, 255, 256, 257, 2047, 2048, 2049, 65536, 65537};
    const int ns[] = {1, 10, 16};
    for (int64_t V : Vs) {
        const SmTree t = sample_tree(V);
        const int64_t P = sample_pow2(V);
        int logP = 0;
        while (((int64_t)1 << logP) < P) ++logP;
        CHECK(t.tiles == (V + SM_TILE - 1) / SM_TILE && t.Vt == (long long)t.tiles * SM_TILE && t.Vt >= V, "V %lld: tiles", (long long)V);
        CHECK(t.top == std::max(logP, SM_TILE_LEVEL), "V %lld: top %d, log2 P %d", (long long)V, t.top, logP);
        CHECK(t.cnt[t.top] == 1, "V %lld: one root", (long long)V);
        // levels: counts, no overlap, aligned to 16 bytes, inside the stride
        std::vector<int> owner(t.node_stride, -1);
        for (int l = SM_SUB_LEVEL; l <= t.top; ++l) {
            const unsigned want = l <= SM_TILE_LEVEL ? (unsigned)(t.Vt >> l) : (unsigned)((t.tiles + (1 << (l - SM_TILE_LEVEL)) - 1) >> (l - SM_TILE_LEVEL));
            CHECK(t.cnt[l] == want, "V %lld level %d: %u nodes, not %u", (long long)V, l, t.cnt[l], want);
            CHECK(t.off[l] % 2 == 0, "V %lld level %d: offset %u not on 16 bytes", (long long)V, l, t.off[l]);
            CHECK((size_t)t.off[l] + t.cnt[l] <= t.node_stride, "V %lld level %d: beyond the stride", (long long)V, l);
            for (unsigned j = 0; j < t.cnt[l] && (size_t)t.off[l] + j < owner.size(); ++j) {
                CHECK(owner[t.off[l] + j] == -1, "V %lld: levels %d and %d overlap", (long long)V, owner[t.off[l] + j], l);
                owner[t.off[l] + j] = l;
            }
        }
        for (int l = 0; l < SM_SUB_LEVEL; ++l) CHECK(t.cnt[l] == 0, "no level below 8 is stored");
        for (int l = t.top + 1; l < SM_MAX_LEVELS; ++l) CHECK(t.cnt[l] == 0, "no level above the root");
        CHECK(t.node_stride % 2 == 0 && (size_t)t.node_stride <= (size_t)(t.Vt / 128) + 2 * SM_MAX_LEVELS, "V %lld: the bound of the header", (long long)V);
        // the low levels of the plain form: 1 .. 7 side by side inside Vt
        for (int l = 1; l < SM_SUB_LEVEL; ++l) {
            CHECK(sample_low_off(t.Vt, l) + (t.Vt >> l) == (l < 7 ? sample_low_off(t.Vt, l + 1) : t.Vt - (t.Vt >> 7)), "low level %d ends where the next starts", l);
            CHECK(sample_low_off(t.Vt, l) % 2 == 0, "low level %d aligned", l);
        }
        CHECK(sample_low_off(t.Vt, 1) == 0 && sample_low_off(t.Vt, 7) + (t.Vt >> 7) <= t.Vt, "the low levels fit in Vt");
        for (int n : ns) {
            CHECK(sample_leaf_elems(n, t.Vt) == (size_t)n * (size_t)t.Vt && sample_node_elems(n, t) == (size_t)n * t.node_stride, "sizes");
            CHECK(sample_work_bytes(n, V) == 8 * (sample_leaf_elems(n, t.Vt) + sample_node_elems(n, t)), "work bytes");
            for (int64_t S : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)1000}) {
                const SmLayout dev = sample_layout(n, S, false, true);
                CHECK(dev.total_bytes == SM_HEAD_BYTES, "a device destination: the head alone");
                for (bool with_w : {false, true}) {
                    const SmLayout h = sample_layout(n, S, true, with_w);
                    CHECK(h.off_total == 0 && h.off_total + 8 * Q_LANES <= h.off_support && h.off_support + 4 * Q_LANES <= h.off_status &&
                              h.off_status + 4 * Q_LANES <= h.off_ids && h.off_ids == SM_HEAD_BYTES,
                          "the head's sections do not overlap");
                    CHECK(h.off_ids + sample_ids_bytes(n, S) <= h.off_w && h.off_w % 8 == 0, "ids before w, w aligned");
                    CHECK(h.total_bytes == h.off_w + (with_w ? sample_w_bytes(n, S) : 0), "total bytes");
                }
            }
        }
    }
    CHECK(sample_draw_blocks(0) == 0 && sample_draw_blocks(1) == 1 && sample_draw_blocks(1024) == 1 && sample_draw_blocks(1025) == 2, "draw blocks");
    CHECK(sample_plain_blocks(1) == 1 && sample_plain_blocks(256) == 1 && sample_plain_blocks(257) == 2, "plain blocks");
    const SmTree big = sample_tree(((int64_t)1 << 31) - 1);
    CHECK(big.top == 31 && big.cnt[31] == 1 && big.cnt[8] == (1u << 23), "the largest window");
}

static void arguments() {
    int32_t ids[1];
    double total[1];
    int32_t status[1];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const uint64_t top = ~(uint64_t)0;
    CHECK(sample_args_ok(nullptr, 0.0, 1, 0, 1, DPPR_DEST_HOST, ids, total, status), "a plain call");
    CHECK(sample_args_ok(nullptr, 0.0, 1, 0, DPPR_SAMPLE_MAX, DPPR_DEST_HOST, ids, total, status), "S at the limit");
    CHECK(!sample_args_ok(nullptr, 0.0, 1, 0, DPPR_SAMPLE_MAX + 1, DPPR_DEST_HOST, ids, total, status), "S above the limit");
    CHECK(!sample_args_ok(nullptr, 0.0, 1, 0, -1, DPPR_DEST_HOST, ids, total, status), "S < 0");
    CHECK(sample_args_ok(nullptr, 0.0, 16, 0, DPPR_SAMPLE_MAX_TOTAL / 16, DPPR_DEST_HOST, ids, total, status), "n * S at the limit");
    CHECK(!sample_args_ok(nullptr, 0.0, 16, 0, DPPR_SAMPLE_MAX_TOTAL / 16 + 1, DPPR_DEST_HOST, ids, total, status), "n * S above the limit");
    CHECK(sample_args_ok(nullptr, 0.0, 10, 0, DPPR_SAMPLE_MAX, DPPR_DEST_HOST, ids, total, status), "10 lanes at the largest S: 10 * 2^20 <= 2^24");
    CHECK(!sample_args_ok(nullptr, 0.0, 0, 0, 1, DPPR_DEST_HOST, ids, total, status) && !sample_args_ok(nullptr, 0.0, 17, 0, 1, DPPR_DEST_HOST, ids, total, status),
          "n outside [1, 16]");
    CHECK(sample_args_ok(nullptr, 0.0, 1, 0, 0, DPPR_DEST_HOST, nullptr, total, status), "S == 0 needs no ids");
    CHECK(!sample_args_ok(nullptr, 0.0, 1, 0, 1, DPPR_DEST_HOST, nullptr, total, status), "NULL ids with S > 0");
    CHECK(!sample_args_ok(nullptr, 0.0, 1, 0, 1, DPPR_DEST_HOST, ids, nullptr, status), "NULL total");
    CHECK(!sample_args_ok(nullptr, 0.0, 1, 0, 1, DPPR_DEST_HOST, ids, total, nullptr), "NULL status");
    CHECK(sample_args_ok(nullptr, 0.0, 1, 0, 1, DPPR_DEST_DEVICE, ids, total, status), "a device destination");
    CHECK(!sample_args_ok(nullptr, 0.0, 1, 0, 1, 2, ids, total, status) && !sample_args_ok(nullptr, 0.0, 1, 0, 1, -1, ids, total, status), "an unknown dest");
    CHECK(sample_args_ok(nullptr, inf, 1, 0, 1, DPPR_DEST_HOST, ids, total, status) && sample_args_ok(nullptr, -0.0, 1, 0, 1, DPPR_DEST_HOST, ids, total, status),
          "min_score >= 0");
    CHECK(!sample_args_ok(nullptr, -1e-300, 1, 0, 1, DPPR_DEST_HOST, ids, total, status) && !sample_args_ok(nullptr, nan, 1, 0, 1, DPPR_DEST_HOST, ids, total, status),
          "min_score negative or NaN");
    CHECK(sample_args_ok(nullptr, 0.0, 1, top - 5, 5, DPPR_DEST_HOST, ids, total, status), "first + S == 2^64 - 1");
    CHECK(!sample_args_ok(nullptr, 0.0, 1, top - 4, 5, DPPR_DEST_HOST, ids, total, status), "first + S wraps to 0");
    CHECK(!sample_args_ok(nullptr, 0.0, 1, top, 1, DPPR_DEST_HOST, ids, total, status) && sample_args_ok(nullptr, 0.0, 1, top, 0, DPPR_DEST_HOST, nullptr, total, status),
          "first at the top: only S == 0");
    dppr_rank_spec_t spec;
    std::memset(&spec, 0, sizeof(spec));
    CHECK(sample_args_ok(&spec, 0.0, 1, 0, 1, DPPR_DEST_HOST, ids, total, status), "the spec of all zeros");
    spec.factor = DPPR_FACTOR_INV_DEG + 1;
    CHECK(!sample_args_ok(&spec, 0.0, 1, 0, 1, DPPR_DEST_HOST, ids, total, status), "an unknown factor");
    spec.factor = DPPR_FACTOR_DEG;
    spec.exclude = 8;
    CHECK(!sample_args_ok(&spec, 0.0, 1, 0, 1, DPPR_DEST_HOST, ids, total, status), "an unknown exclude bit");
    spec.exclude = 7;
    spec.mask = DPPR_MASK_DENY + 1;
    CHECK(!sample_args_ok(&spec, 0.0, 1, 0, 1, DPPR_DEST_HOST, ids, total, status), "an unknown mask");
    CHECK(sample_form_ok(0) && sample_form_ok(1) && !sample_form_ok(2) && !sample_form_ok(-1), "forms");
}

static void uniform_and_rule() {
    CHECK(sample_uniform(0u, 0u) == 0.0, "the smallest uniform");
    const double hi = sample_uniform(0xffffffffu, 0xffffffffu);
    CHECK(hi < 1.0 && hi == 1.0 - 0x1p-53, "the largest uniform is 1 - 2^-53");
    CHECK(sample_uniform(0x80000000u, 0u) == 0.5 && sample_uniform(0u, 0x7ffu) == 0.0 && sample_uniform(0u, 0x800u) == 0x1p-53, "53 bits, the low 11 dropped");
    const Philox4 r = walk_philox(5u, 0u, 3u, SM_DOMAIN, 7u, 0u);
    CHECK(sample_u(5, 3, 7) == sample_uniform(r.x0, r.x1), "the counter of a draw");
    const Philox4 r2 = walk_philox(0xfffffffeu, 1u, 0u, SM_DOMAIN, 0x89abcdefu, 0x01234567u);
    CHECK(sample_u(0x1fffffffeull, 0, 0x0123456789abcdefull) == sample_uniform(r2.x0, r2.x1), "64-bit draw numbers and seeds split low word first");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(sample_weight(0.5, 0.0) == 0.5 && sample_weight(0.5, 0.5) == 0.0 && sample_weight(-1.0, 0.0) == 0.0 && sample_weight(nan, 0.0) == 0.0 &&
              !std::signbit(sample_weight(-0.0, 0.0)) && sample_weight(inf, 0.0) == inf,
          "the weight rule");
    CHECK(sample_status(0.0) == DPPR_SAMPLE_EMPTY && sample_status(1e-300) == DPPR_SAMPLE_OK && sample_status(inf) == DPPR_SAMPLE_NONFINITE &&
              sample_status(nan) == DPPR_SAMPLE_NONFINITE,
          "statuses");
    double x = 0.6;
    CHECK(sample_step(x, 0.5, 0.25) && x == 0.6 - 0.5, "right: x >= L and R > 0");
    x = 0.6;
    CHECK(!sample_step(x, 0.5, 0.0) && x == 0.6, "x >= L but R == 0: left, x untouched");
    x = 0.25;
    CHECK(!sample_step(x, 0.5, 0.25) && x == 0.25, "x < L: left");
    x = 0.5;
    CHECK(sample_step(x, 0.5, 0.25) && x == 0.0, "x == L goes right");
}

// the hand-worked case of the issue, and a draw whose x is the root itself
static void hand_case() {
    const double w[5] = {0.5, 0.0, 0.25, 0.125, 0.125};
    std::vector<std::vector<double>> lv;
    sample_tree_ref(w, 5, lv);
    CHECK(lv.size() == 4 && lv[0].size() == 8 && lv[3][0] == 1.0, "8 leaves, root 1.0");
    CHECK(lv[1][0] == 0.5 && lv[1][1] == 0.375 && lv[1][2] == 0.125 && lv[1][3] == 0.0 && lv[2][0] == 0.875 && lv[2][1] == 0.125, "the levels");
    CHECK(sample_descend_ref(lv, 0.6) == 2 && sample_descend_ref(lv, 0.8) == 3, "0.6 -> 2, 0.8 -> 3: left at the root");
    CHECK(sample_descend_ref(lv, 0.9) == 4 && sample_descend_ref(lv, 0.95) == 4, "0.9 and 0.95 -> 4: right at the root, then left of a +0.0 sibling twice");
    CHECK(sample_descend_ref(lv, 0.0) == 0 && sample_descend_ref(lv, 0.49) == 0 && sample_descend_ref(lv, 0.5) == 2, "the left edge of a leaf belongs to it");
    CHECK(sample_descend_ref(lv, 1.0) == 4, "x == root ends on the last positive leaf, not on padding");
    const double one[3] = {0.0, 0.0, 0.3};
    sample_tree_ref(one, 3, lv);
    for (uint64_t j = 0; j < 100; ++j) CHECK(sample_draw_ref(lv, j, 2, 99) == 2, "one positive leaf is every draw");
    const double none[3] = {0.0, 0.0, 0.0};
    sample_tree_ref(none, 3, lv);
    CHECK(sample_draw_ref(lv, 0, 0, 0) == -1, "an empty lane draws -1");
}

// exact dyadic weights: every sum is exact, so the leaf of x is the one whose half-open interval of the prefix sums holds x
static void against_a_linear_scan() {
    for (int round = 0; round < 200; ++round) {
        const int64_t V = 1 + (int64_t)(rng() % 300);
        std::vector<double> w((size_t)V);
        bool any = false;
        for (auto &x : w) {
            const uint64_t r = rng();
            x = (r & 3) == 0 ? 0.0 : (double)(1 + (r >> 8) % 1024) * 0x1p-20; // multiples of 2^-20 below 2^-10: 300 of them sum exactly
            any = any || x > 0.0;
        }
        if (!any) w[0] = 0x1p-20;
        std::vector<std::vector<double>> lv;
        sample_tree_ref(w.data(), V, lv);
        double sum = 0.0;
        for (double x : w) sum += x;
        CHECK(lv.back()[0] == sum, "the root is the exact sum");
        for (uint64_t j = 0; j < 500; ++j) {
            const double x = sample_scale(sample_u(j, (uint32_t)(round % 16), 42), sum);
            int64_t want = -1;
            double acc = 0.0;
            for (int64_t v = 0; v < V; ++v) {
                if (w[(size_t)v] > 0.0 && x >= acc && x < acc + w[(size_t)v]) want = v;
                acc += w[(size_t)v];
            }
            if (want < 0) // (x rounded up to the sum: the last positive leaf)
                for (int64_t v = V - 1; v >= 0 && want < 0; --v)
                    if (w[(size_t)v] > 0.0) want = v;
            const int64_t got = sample_draw_ref(lv, j, (uint32_t)(round % 16), 42);
            CHECK(got == want, "round %d draw %llu: leaf %lld, the scan says %lld", round, (unsigned long long)j, (long long)got, (long long)want);
        }
    }
}

// 10^5 random trees with zeros and weights of very different size: every node a descent enters is positive, whatever x is
static void never_a_zero_node() {
    for (int round = 0; round < 100000; ++round) {
        const int64_t V = 1 + (int64_t)(rng() % 40);
        std::vector<double> w((size_t)V);
        bool any = false;
        for (auto &x : w) {
            const uint64_t r = rng();
            x = (r & 1) ? 0.0 : std::ldexp((double)((r >> 11) | 1), -53 - (int)((r >> 2) % 60));
            any = any || x > 0.0;
        }
        if (!any) w[(size_t)(rng() % (uint64_t)V)] = 1.0;
        std::vector<std::vector<double>> lv;
        sample_tree_ref(w.data(), V, lv);
        const double root = lv.back()[0];
        const double xs[4] = {0.0, root, sample_scale(sample_uniform((uint32_t)rng(), (uint32_t)rng()), root), std::nextafter(root, 0.0)};
        for (double x0 : xs) {
            double x = x0;
            int64_t k = 0;
            for (size_t l = lv.size() - 1; l > 0; --l) {
                k = 2 * k + (sample_step(x, lv[l - 1][(size_t)(2 * k)], lv[l - 1][(size_t)(2 * k + 1)]) ? 1 : 0);
                if (!(lv[l - 1][(size_t)k] > 0.0)) {
                    CHECK(false, "round %d: entered a node of value %g at level %zu", round, lv[l - 1][(size_t)k], l - 1);
                    l = 1;
                }
            }
            CHECK(k < V && w[(size_t)k] > 0.0, "round %d: the leaf weighs nothing", round);
        }
    }
}

// The stored shape gives the definition's tree: tiles of 2048 padded with +0.0, a missing sibling read as +0.0, and -- where
// P < 2048 -- levels above the definition's root that the descent passes through on the left.
static void stored_shape_is_the_definition() {
    const int64_t Vs[] = {1, 5, 257, 2049, 5001, 70001};
    for (int64_t V : Vs) {
        std::vector<double> w((size_t)V);
        for (auto &x : w) {
            const uint64_t r = rng();
            x = (r & 3) == 0 ? 0.0 : std::ldexp((double)((r >> 11) | 1), -53 - (int)((r >> 2) % 30));
        }
        w[(size_t)(V - 1)] = 0.25; // (the last id is positive: the last tile and subtile are partial and matter)
        std::vector<std::vector<double>> def;
        sample_tree_ref(w.data(), V, def);
        const SmTree t = sample_tree(V);
        std::vector<std::vector<double>> st((size_t)t.top + 1);
        st[0].assign((size_t)t.Vt, 0.0);
        std::copy(w.begin(), w.end(), st[0].begin());
        for (int l = 1; l <= t.top; ++l) {
            const size_t c = l <= SM_TILE_LEVEL ? (size_t)(t.Vt >> l) : t.cnt[l];
            st[(size_t)l].resize(c);
            for (size_t j = 0; j < c; ++j) {
                const std::vector<double> &lo = st[(size_t)l - 1];
                st[(size_t)l][j] = lo[2 * j] + (2 * j + 1 < lo.size() ? lo[2 * j + 1] : 0.0);
            }
        }
        uint64_t a, b;
        std::memcpy(&a, &st[(size_t)t.top][0], 8);
        std::memcpy(&b, &def.back()[0], 8);
        CHECK(a == b, "V %lld: the stored root is the definition's bit for bit", (long long)V);
        for (size_t l = 0; l < def.size() && l < st.size(); ++l)
            for (size_t j = 0; j < std::min(def[l].size(), st[l].size()); ++j)
                if (std::memcmp(&def[l][j], &st[l][j], 8) != 0) {
                    CHECK(false, "V %lld: node %zu of level %zu differs", (long long)V, j, l);
                    break;
                }
        for (uint64_t j = 0; j < 2000; ++j) {
            double x = sample_scale(sample_u(j, 1, 7), def.back()[0]);
            const int64_t want = sample_draw_ref(def, j, 1, 7);
            size_t k = 0;
            for (int l = t.top; l >= 1; --l) {
                const std::vector<double> &lo = st[(size_t)l - 1];
                k = 2 * k + (sample_step(x, lo[2 * k], 2 * k + 1 < lo.size() ? lo[2 * k + 1] : 0.0) ? 1 : 0);
            }
            CHECK((int64_t)k == want, "V %lld draw %llu: the stored shape gives %zu, the definition %lld", (long long)V, (unsigned long long)j, k, (long long)want);
        }
    }
}

int main() {
    shapes();
    arguments();
    uniform_and_rule();
    hand_case();
    against_a_linear_scan();
    never_a_zero_node();
    stored_shape_is_the_definition();
    std::printf("sample_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
