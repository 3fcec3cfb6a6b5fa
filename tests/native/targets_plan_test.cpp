// targets_plan_test.cpp -- dynamicppr_amd/csrc/dppr_targets_plan.hpp on the CPU: every rejection of the argument check at its
// limit, the host mirror (external ids ascending), the device table through an ext -> int lookup (internal ids ascending within
// a lane, the weights following their ids), the binary search the device does, the table under a permutation against a rebuild,
// replace / add / remove through the lane maps of dppr_churn_plan.hpp, the dppr_group_sources projection, the packed block and
// the listing with its capacity rule. Every array is exactly as long as the code may touch (the sanitizers watch the bounds).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_churn_plan.hpp"
#include "../../dynamicppr_amd/csrc/dppr_targets_plan.hpp"

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

static void arguments() {
    const int64_t V = 100;
    {
        const std::vector<int64_t> off = {0, 1, 3};
        const std::vector<int32_t> ids = {5, 99, 0};
        const std::vector<double> w = {1.0, 0.25, 1e-300};
        CHECK(tg_check(off.data(), ids.data(), w.data(), 2, V) == TG_OK, "a valid group");
        CHECK(tg_check(off.data(), ids.data(), w.data(), 0, V) == TG_BAD_N && tg_check(off.data(), ids.data(), w.data(), 17, V) == TG_BAD_N &&
                  tg_check(off.data(), ids.data(), w.data(), -1, V) == TG_BAD_N,
              "n");
        CHECK(tg_check(nullptr, ids.data(), w.data(), 2, V) == TG_NULL && tg_check(off.data(), nullptr, w.data(), 2, V) == TG_NULL &&
                  tg_check(off.data(), ids.data(), nullptr, 2, V) == TG_NULL,
              "NULL");
    }
    {
        const std::vector<int32_t> ids = {1, 2, 3};
        const std::vector<double> w = {1, 1, 1};
        const std::vector<int64_t> not0 = {1, 2, 3}, down = {0, 2, 1}, empty = {0, 0, 3}, empty_last = {0, 3, 3};
        CHECK(tg_check(not0.data(), ids.data(), w.data(), 2, V) == TG_BAD_OFFSETS, "offsets start at 0");
        CHECK(tg_check(down.data(), ids.data(), w.data(), 2, V) == TG_BAD_OFFSETS, "offsets decrease");
        CHECK(tg_check(empty.data(), ids.data(), w.data(), 2, V) == TG_BAD_SIZE && tg_check(empty_last.data(), ids.data(), w.data(), 2, V) == TG_BAD_SIZE,
              "an empty lane");
    }
    { // the size limit itself and one more (ids unique: V large enough)
        const int64_t m = TG_SET_MAX + 1;
        std::vector<int32_t> ids((size_t)m);
        std::iota(ids.begin(), ids.end(), 0);
        const std::vector<double> w((size_t)m, 0.5);
        CHECK(tg_check_lane(ids.data(), w.data(), TG_SET_MAX, m) == TG_OK, "DPPR_TARGET_SET_MAX seeds");
        CHECK(tg_check_lane(ids.data(), w.data(), m, m) == TG_BAD_SIZE && tg_check_lane(ids.data(), w.data(), 0, m) == TG_BAD_SIZE, "one more, none");
        const std::vector<int64_t> off = {0, m};
        CHECK(tg_check(off.data(), ids.data(), w.data(), 1, m) == TG_BAD_SIZE, "... through the group check");
    }
    {
        const std::vector<double> w = {1, 1};
        const std::vector<int32_t> neg = {3, -1}, big = {3, 100}, dup = {7, 7}, ok = {99, 0};
        CHECK(tg_check_lane(neg.data(), w.data(), 2, V) == TG_BAD_ID && tg_check_lane(big.data(), w.data(), 2, V) == TG_BAD_ID, "ids in [0, V)");
        CHECK(tg_check_lane(dup.data(), w.data(), 2, V) == TG_DUP_ID && tg_check_lane(ok.data(), w.data(), 2, V) == TG_OK, "an id twice");
        // the same id in different lanes is fine
        const std::vector<int64_t> off = {0, 1, 2};
        CHECK(tg_check(off.data(), dup.data(), w.data(), 2, V) == TG_OK, "the same id in two lanes");
        CHECK(tg_check_lane(nullptr, w.data(), 2, V) == TG_NULL, "NULL lane");
    }
    {
        const std::vector<int32_t> ids = {1, 2};
        for (double bad : {0.0, -0.0, -1.0, std::nan(""), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()}) {
            const std::vector<double> w = {1.0, bad};
            CHECK(tg_check_lane(ids.data(), w.data(), 2, V) == TG_BAD_WEIGHT, "weight %g", bad);
        }
        const std::vector<double> w = {std::numeric_limits<double>::denorm_min(), std::numeric_limits<double>::max()};
        CHECK(tg_check_lane(ids.data(), w.data(), 2, V) == TG_OK, "the smallest and the largest weight");
    }
    for (int c = TG_OK; c <= TG_BAD_WEIGHT; ++c) CHECK(std::strlen(tg_check_text((TgCheck)c)) > 0, "a text for every rejection");
}

static TargetSets three_lanes() {
    const std::vector<int64_t> off = {0, 1, 4, 6};
    const std::vector<int32_t> ids = {9, 30, 10, 20, 9, 2};
    const std::vector<double> w = {1.0, 0.3, 0.1, 0.2, 0.5, 0.5};
    return tg_build(off.data(), ids.data(), w.data(), 3);
}

static void mirror_and_projection() {
    const TargetSets ts = three_lanes();
    CHECK(ts.n == 3 && ts.total() == 6, "sizes");
    CHECK(ts.lane[1][0].id == 10 && ts.lane[1][1].id == 20 && ts.lane[1][2].id == 30 && ts.lane[1][0].w == 0.1 && ts.lane[1][2].w == 0.3,
          "external ids ascending, the weights with them");
    CHECK(ts.lane[2][0].id == 2 && ts.lane[2][1].id == 9, "lane 2");
    CHECK(tg_is_source(ts.lane[0]) && !tg_is_source(ts.lane[1]) && !tg_is_source(ts.lane[2]) && tg_has_set(ts), "source lanes");
    const std::vector<TgSeed> half = {{4, 0.5}};
    CHECK(!tg_is_source(half) && tg_is_source(tg_source_lane(4)), "one seed of another weight is a set");
    int32_t src[3];
    tg_sources(ts, src);
    CHECK(src[0] == 9 && src[1] == -1 && src[2] == -1, "projection");
    TargetSets plain;
    plain.n = 2;
    plain.lane[0] = tg_source_lane(3);
    plain.lane[1] = tg_source_lane(3);
    CHECK(!tg_has_set(plain), "a group of sources");
    // listing: true offsets always, arrays only when cap suffices
    int64_t off[TG_LANES + 1];
    std::vector<int32_t> ids(6, -7);
    std::vector<double> w(6, -7.0);
    tg_list(ts, off, nullptr, nullptr, 0);
    CHECK(off[0] == 0 && off[1] == 1 && off[2] == 4 && off[3] == 6 && off[TG_LANES] == 6, "size query");
    tg_list(ts, off, ids.data(), w.data(), 5);
    CHECK(off[TG_LANES] == 6 && ids[0] == -7 && w[5] == -7.0, "short cap: nothing written");
    tg_list(ts, off, ids.data(), w.data(), 6);
    const int32_t want[6] = {9, 10, 20, 30, 2, 9};
    CHECK(std::equal(ids.begin(), ids.end(), want) && w[1] == 0.1 && w[4] == 0.5, "the listing");
}

static void table() {
    const TargetSets ts = three_lanes();
    // ext -> int reverses the order inside [0, 100)
    auto e2i = [](int32_t ext) { return 99 - ext; };
    TgTable t = tg_table(ts, e2i);
    CHECK(t.total() == 6 && t.off[0] == 0 && t.off[1] == 1 && t.off[2] == 4 && t.off[3] == 6 && t.off[TG_LANES] == 6, "offsets, empty lanes behind");
    CHECK(t.ids[1] == 69 && t.ids[2] == 79 && t.ids[3] == 89 && t.w[1] == 0.3 && t.w[2] == 0.2 && t.w[3] == 0.1, "internal ids ascending, weights follow");
    for (int lane = 0; lane < 3; ++lane)
        for (int v = 0; v < 100; ++v) {
            double want = 0.0;
            for (const TgSeed &s : ts.lane[lane])
                if (e2i(s.id) == v) want = s.w;
            CHECK(tg_weight_at(t, lane, v) == want, "lookup lane %d vertex %d", lane, v);
        }
    CHECK(tg_weight_at(t, 5, 3) == 0.0 && tg_weight_at(t, TG_LANES - 1, 3) == 0.0, "an empty lane holds nothing");
    // the packed block
    std::vector<unsigned char> blob(tg_bytes(t.total()));
    tg_pack(t, blob.data());
    CHECK(tg_bytes(6) == 8 * 6 + 4 * 17 + 4 * 6 + 4 && tg_off_at(6) % 4 == 0 && tg_ids_at(6) % 4 == 0 && tg_w_at() == 0, "sections");
    double w1;
    int o2, i3;
    std::memcpy(&w1, blob.data() + tg_w_at() + 8, 8);
    std::memcpy(&o2, blob.data() + tg_off_at(6) + 8, 4);
    std::memcpy(&i3, blob.data() + tg_ids_at(6) + 12, 4);
    CHECK(w1 == 0.3 && o2 == 4 && i3 == 89, "contents");
    // a permutation against a rebuild in the new numbering
    std::mt19937 rng(5);
    std::vector<int32_t> perm(100);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    TgTable moved = t;
    tg_remap(moved, perm.data());
    const TgTable rebuilt = tg_table(ts, [&](int32_t ext) { return perm[(size_t)e2i(ext)]; });
    CHECK(moved.ids == rebuilt.ids && moved.w == rebuilt.w && std::equal(moved.off, moved.off + TG_LANES + 1, rebuilt.off), "remap == rebuild");
    for (int lane = 0; lane < 3; ++lane)
        for (int k = moved.off[lane] + 1; k < moved.off[lane + 1]; ++k) CHECK(moved.ids[(size_t)k - 1] < moved.ids[(size_t)k], "sorted again");
}

static void random_tables() {
    std::mt19937 rng(11);
    for (int trial = 0; trial < 50; ++trial) {
        const int V = 50 + (int)(rng() % 400), n = 1 + (int)(rng() % 16);
        std::vector<int64_t> off(1, 0);
        std::vector<int32_t> ids;
        std::vector<double> w;
        std::vector<int32_t> all((size_t)V);
        std::iota(all.begin(), all.end(), 0);
        for (int i = 0; i < n; ++i) {
            const int m = 1 + (int)(rng() % (unsigned)std::min(V, 60));
            std::shuffle(all.begin(), all.end(), rng);
            for (int k = 0; k < m; ++k) {
                ids.push_back(all[(size_t)k]);
                w.push_back(1.0 + (double)(rng() % 1000) / 7.0);
            }
            off.push_back((int64_t)ids.size());
        }
        CHECK(tg_check(off.data(), ids.data(), w.data(), n, V) == TG_OK, "random group");
        const TargetSets ts = tg_build(off.data(), ids.data(), w.data(), n);
        std::vector<int32_t> e2i((size_t)V);
        std::iota(e2i.begin(), e2i.end(), 0);
        std::shuffle(e2i.begin(), e2i.end(), rng);
        const TgTable t = tg_table(ts, [&](int32_t ext) { return e2i[(size_t)ext]; });
        for (int i = 0; i < n; ++i) {
            std::vector<double> h((size_t)V, 0.0);
            for (int64_t k = off[(size_t)i]; k < off[(size_t)i + 1]; ++k) h[(size_t)e2i[(size_t)ids[(size_t)k]]] = w[(size_t)k];
            for (int v = 0; v < V; ++v) CHECK(tg_weight_at(t, i, v) == h[(size_t)v], "trial %d lane %d vertex %d", trial, i, v);
        }
        std::vector<int64_t> lo(TG_LANES + 1);
        std::vector<int32_t> li(ids.size());
        std::vector<double> lw(w.size());
        tg_list(ts, lo.data(), li.data(), lw.data(), (int64_t)ids.size());
        for (int i = 0; i < n; ++i) {
            CHECK(lo[(size_t)i + 1] == off[(size_t)i + 1], "offsets");
            CHECK(std::is_sorted(li.begin() + lo[(size_t)i], li.begin() + lo[(size_t)i + 1]), "ascending");
        }
    }
}

static void churn() {
    const TargetSets ts = three_lanes(); // source 9 | {10, 20, 30} | {2, 9}
    { // remove lane 0: the sets move down with their lanes
        const ChurnPlan pl = churn_plan(CHURN_REMOVE, 3, 4, 0, false, false);
        const TargetSets out = tg_relane(ts, pl.map, pl.n, pl.lane, {});
        CHECK(out.n == 2 && out.lane[0].size() == 3 && out.lane[0][0].id == 10 && out.lane[1].size() == 2 && out.lane[1][1].id == 9 && out.lane[2].empty(), "remove");
        int32_t src[2];
        tg_sources(out, src);
        CHECK(src[0] == -1 && src[1] == -1, "no source left");
    }
    { // remove the middle lane
        const ChurnPlan pl = churn_plan(CHURN_REMOVE, 3, 4, 1, false, false);
        const TargetSets out = tg_relane(ts, pl.map, pl.n, pl.lane, {});
        CHECK(out.n == 2 && tg_is_source(out.lane[0]) && out.lane[1].size() == 2 && out.lane[1][0].id == 2, "remove the middle lane");
    }
    { // add a source: lane 3
        const ChurnPlan pl = churn_plan(CHURN_ADD, 3, 4, -1, false, false);
        const TargetSets out = tg_relane(ts, pl.map, pl.n, pl.lane, tg_source_lane(77));
        CHECK(out.n == 4 && pl.lane == 3 && tg_is_source(out.lane[3]) && out.lane[3][0].id == 77 && out.lane[1].size() == 3, "add");
    }
    { // replace a set lane by a source, then the other one: a group of sources again
        ChurnPlan pl = churn_plan(CHURN_REPLACE, 3, 4, 1, false, false);
        TargetSets out = tg_relane(ts, pl.map, pl.n, pl.lane, tg_source_lane(5));
        CHECK(out.n == 3 && tg_is_source(out.lane[1]) && out.lane[1][0].id == 5 && tg_has_set(out), "replace by a source");
        pl = churn_plan(CHURN_REPLACE, 3, 4, 2, false, false);
        out = tg_relane(out, pl.map, pl.n, pl.lane, tg_source_lane(6));
        CHECK(!tg_has_set(out), "the last set lane became a source");
    }
    { // replace by a set
        const std::vector<int32_t> ids = {50, 40};
        const std::vector<double> w = {2.0, 3.0};
        const ChurnPlan pl = churn_plan(CHURN_REPLACE, 3, 4, 0, false, false);
        const TargetSets out = tg_relane(ts, pl.map, pl.n, pl.lane, tg_lane(ids.data(), w.data(), 2));
        CHECK(out.lane[0].size() == 2 && out.lane[0][0].id == 40 && out.lane[0][0].w == 3.0 && out.lane[2].size() == 2, "replace by a set");
    }
}

int main() {
    arguments();
    mirror_and_projection();
    table();
    random_tables();
    churn();
    std::printf("targets plan: %d failures\n", failures);
    return failures ? 1 : 0;
}
