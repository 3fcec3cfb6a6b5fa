// CPU test driver for dynamicppr_amd/csrc/dppr_churn_plan.hpp (what replacing, adding or removing a source does to a
// group's interleaved rows): every source count 1..16, every operation, every index (and some outside), both row
// layouts, against a plain restatement written here.   churn_test
#include <cstdio>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_churn_plan.hpp"

static int fails = 0;
static long long checked = 0;
#define CHECK(c, ...) do { ++checked; if (!(c)) { if (fails++ < 10) { printf("FAILED %s (line %d): ", #c, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// rows hold the sources and at most one padding double, never fewer than 2 (dppr_multi.hpp); the full-row layout: 8 or 16
static int width(int n, bool full) {
    if (full) return n <= 8 ? 8 : 16;
    int w = 2;
    while (w < n) w += 2;
    return w;
}

int main() {
    for (int full = 0; full < 2; ++full)
        for (int wide = 0; wide < 2; ++wide)
            for (int n = 1; n <= 16; ++n)
                for (int op = 0; op < 3; ++op)
                    for (int index = -2; index <= 17; ++index) {
                        const int gw = width(n, full);
                        const dppr::ChurnPlan pl = dppr::churn_plan((dppr::ChurnOp)op, n, gw, index, full, wide);
                        const bool in_range = index >= 0 && index < n;
                        const bool admissible = op == dppr::CHURN_ADD ? n < 16 : op == dppr::CHURN_REMOVE ? in_range && n > 1 : in_range;
                        CHECK(pl.ok == admissible, "op %d n %d index %d: ok %d", op, n, index, (int)pl.ok);
                        if (!pl.ok || !admissible) continue;
                        // the sources afterwards as a list of old lanes (-1: the new one)
                        std::vector<int> lanes;
                        for (int j = 0; j < n; ++j) lanes.push_back(j);
                        int fresh = -1;
                        if (op == dppr::CHURN_ADD) { lanes.push_back(-1); fresh = n; }
                        if (op == dppr::CHURN_REPLACE) { lanes[(size_t)index] = -1; fresh = index; }
                        if (op == dppr::CHURN_REMOVE) lanes.erase(lanes.begin() + index);
                        const int n2 = (int)lanes.size(), gw2 = width(n2, full);
                        CHECK(pl.n == n2 && pl.gw == gw2 && pl.spl == (gw2 > 8 ? 2 : 1), "op %d n %d index %d: n %d gw %d spl %d", op, n, index, pl.n, pl.gw, pl.spl);
                        CHECK(pl.gw % 2 == 0 && pl.gw >= pl.n && pl.gw >= 2 && pl.gw <= 16, "row width %d for %d sources", pl.gw, pl.n);
                        CHECK(pl.lane == fresh, "op %d n %d index %d: lane %d, expected %d", op, n, index, pl.lane, fresh);
                        int last = -1;
                        for (int j = 0; j < dppr::CHURN_LANES; ++j) {
                            const int want = j < n2 ? lanes[(size_t)j] : -1; // padding and lanes beyond the row: zeros
                            CHECK(pl.map[j] == want, "op %d n %d index %d: map[%d] = %d, expected %d", op, n, index, j, pl.map[j], want);
                            if (pl.map[j] >= 0) { // survivors in their old order, each once
                                CHECK(pl.map[j] > last && pl.map[j] < n, "map not increasing at %d", j);
                                last = pl.map[j];
                            }
                        }
                        const bool moved = op == dppr::CHURN_REMOVE || gw2 != gw; // (a shift inside the same width is a remap too)
                        CHECK(pl.relayout == moved, "op %d n %d index %d: relayout %d", op, n, index, (int)pl.relayout);
                        CHECK(pl.recut == (gw2 > 8 && !wide), "op %d n %d: recut %d (wide %d, gw %d)", op, n, (int)pl.recut, wide, gw2);
                    }
    // the cases the engine's documentation names
    CHECK(!dppr::churn_plan(dppr::CHURN_ADD, 1, 2, 0, false, false).relayout, "1 -> 2 fills the padding lane");
    CHECK(dppr::churn_plan(dppr::CHURN_ADD, 2, 2, 0, false, false).gw == 4, "2 -> 3 doubles the row");
    CHECK(!dppr::churn_plan(dppr::CHURN_ADD, 7, 8, 0, false, false).relayout, "7 -> 8 fills the padding lane");
    const dppr::ChurnPlan nine = dppr::churn_plan(dppr::CHURN_ADD, 8, 8, 0, false, false);
    CHECK(nine.gw == 10 && nine.spl == 2 && nine.relayout && nine.recut, "8 -> 9 switches the lane split");
    const dppr::ChurnPlan eight = dppr::churn_plan(dppr::CHURN_REMOVE, 9, 10, 4, false, true);
    CHECK(eight.gw == 8 && eight.spl == 1 && !eight.recut, "9 -> 8 goes back to one double per lane");
    CHECK(dppr::churn_plan(dppr::CHURN_ADD, 10, 10, 0, false, true).gw == 12, "10 -> 11: rows of 80 -> 96 bytes");
    printf("%lld checks, %d failures\n", checked, fails);
    return fails ? 1 : 0;
}
