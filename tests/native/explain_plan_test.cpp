// explain_plan_test.cpp -- dynamicppr_amd/csrc/dppr_explain_plan.hpp on the CPU: every rejection of a call's arguments at its
// limit, the hook's values, the layout of the result block for every combination of outputs -- planes that do not overlap, double
// planes at multiples of 8, room only for what is asked, the ids behind the bytes that are copied --, the memo decision and its
// size, and the grid that gives every (query, lane) pair exactly one wave.
// Every array is exactly as long as the code may touch (the sanitizers watch the bounds).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_explain_plan.hpp"

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
    std::vector<int32_t> ids(DPPR_EXPLAIN_MAX_M, 7), over(DPPR_EXPLAIN_MAX_M + 1, 7);
    dppr_explain_out_t out{};
    CHECK(ex_args_ok(ids.data(), 4, 3, 16, V, &out), "a plain call");
    CHECK(ex_args_ok(ids.data(), DPPR_EXPLAIN_MAX_M, DPPR_EXPLAIN_MAX_F, DPPR_EXPLAIN_MAX_DEPTH, V, &out), "every limit itself");
    CHECK(!ex_args_ok(over.data(), DPPR_EXPLAIN_MAX_M + 1, 3, 16, V, &out), "m above the limit");
    CHECK(!ex_args_ok(ids.data(), -1, 3, 16, V, &out), "m < 0");
    CHECK(!ex_args_ok(ids.data(), 4, DPPR_EXPLAIN_MAX_F + 1, 16, V, &out) && !ex_args_ok(ids.data(), 4, -1, 16, V, &out), "f outside");
    CHECK(!ex_args_ok(ids.data(), 4, 3, DPPR_EXPLAIN_MAX_DEPTH + 1, V, &out) && !ex_args_ok(ids.data(), 4, 3, -1, V, &out), "depth outside");
    CHECK(!ex_args_ok(ids.data(), 4, 0, 0, V, &out), "f + depth == 0");
    CHECK(ex_args_ok(ids.data(), 4, 1, 0, V, &out) && ex_args_ok(ids.data(), 4, 0, 1, V, &out), "f + depth == 1");
    CHECK(ex_args_ok(nullptr, 0, 3, 16, V, nullptr), "m == 0 needs neither ids nor out");
    CHECK(!ex_args_ok(nullptr, 0, 0, 0, V, nullptr), "m == 0 does not excuse f + depth == 0");
    CHECK(!ex_args_ok(nullptr, 1, 3, 16, V, &out), "NULL ids with m > 0");
    CHECK(!ex_args_ok(ids.data(), 1, 3, 16, V, nullptr), "NULL out with m > 0");
    std::vector<int32_t> edge = {0, (int32_t)V - 1};
    CHECK(ex_args_ok(edge.data(), 2, 3, 16, V, &out), "ids at both ends of [0, V)");
    edge[1] = (int32_t)V;
    CHECK(!ex_args_ok(edge.data(), 2, 3, 16, V, &out), "an id == V");
    edge[1] = -1;
    CHECK(!ex_args_ok(edge.data(), 2, 3, 16, V, &out), "an id < 0");
    CHECK(ex_args_ok(edge.data(), 1, 3, 16, V, &out), "only m ids are read");

    CHECK(ex_hook_ok(-1, 64) && ex_hook_ok(0, 1) && ex_hook_ok(1, 7), "the hook's values");
    CHECK(!ex_hook_ok(-2, 64) && !ex_hook_ok(2, 64) && !ex_hook_ok(0, 0) && !ex_hook_ok(0, 65) && !ex_hook_ok(0, -1), "the hook's rejections");
}

static void which_bits() {
    int32_t i = 0;
    double d = 0;
    dppr_explain_out_t out{};
    CHECK(ex_which(nullptr, 3, 3) == 0 && ex_which(&out, 3, 3) == 0, "nothing asked");
    out.deg = &i;
    out.nbr = &i;
    out.nbr_c = &d;
    out.path_c = &d;
    out.len = &i;
    CHECK(ex_which(&out, 3, 3) == (EX_DEG | EX_NBR | EX_NBR_C | EX_PATH_C | EX_LEN), "the pointers given");
    CHECK(ex_which(&out, 0, 3) == (EX_DEG | EX_PATH_C | EX_LEN), "f == 0: no plane of f entries");
    CHECK(ex_which(&out, 3, 0) == (EX_DEG | EX_NBR | EX_NBR_C | EX_LEN), "depth == 0: path_c is unused");
    CHECK((EX_FIRST & EX_WALK) == 0 && (EX_FIRST | EX_WALK) == (1u << 12) - 1, "the two kernels share no output and miss none");
}

struct Plane {
    uint32_t bit;
    size_t off, bytes;
    bool dbl;
};

static void layout_of(int m, int n, int f, int depth, uint32_t which) {
    const ExplainLayout l = ex_layout(m, n, f, depth, which);
    const size_t mn = (size_t)m * n;
    const Plane planes[] = {
        {EX_SELF, l.off_self, 8 * mn, true},
        {EX_NBR_C, l.off_nbr_c, 8 * mn * f, true},
        {EX_PATH_P, l.off_path_p, 8 * mn * (depth + 1), true},
        {EX_PATH_C, l.off_path_c, 8 * mn * depth, true},
        {EX_DEG, l.off_deg, 4 * (size_t)m, false},
        {EX_DISTINCT, l.off_distinct, 4 * (size_t)m, false},
        {EX_NBR_COUNT, l.off_nbr_count, 4 * mn, false},
        {EX_NBR, l.off_nbr, 4 * mn * f, false},
        {EX_NBR_MULT, l.off_nbr_mult, 4 * mn * f, false},
        {EX_LEN, l.off_len, 4 * mn, false},
        {EX_END, l.off_end, 4 * mn, false},
        {EX_PATH, l.off_path, 4 * mn * (depth + 1), false},
    };
    std::vector<unsigned char> owner(l.total_bytes, 0); // every byte belongs to one plane at the most
    size_t asked = 0;
    for (const Plane &p : planes) {
        if (!(which & p.bit)) continue;
        asked += p.bytes;
        CHECK(p.off % (p.dbl ? 8 : 4) == 0, "alignment of plane %u at %zu (m %d n %d f %d depth %d which %x)", p.bit, p.off, m, n, f, depth, which);
        CHECK(p.off + p.bytes <= l.copy_bytes, "plane %u ends inside the copy", p.bit);
        for (size_t b = p.off; b < p.off + p.bytes && b < owner.size(); ++b) {
            CHECK(owner[b] == 0, "byte %zu has two owners (which %x)", b, which);
            owner[b] = 1;
        }
    }
    CHECK(l.copy_bytes == asked, "room only for what is asked: %zu != %zu", l.copy_bytes, asked);
    CHECK(l.off_ids == l.copy_bytes && l.off_ids % 4 == 0, "the ids behind the copy");
    CHECK(l.total_bytes >= l.off_ids + 4 * (size_t)m && l.total_bytes % 8 == 0 && l.total_bytes >= 8, "the block holds the ids");
}

static void layouts() {
    const int ms[] = {0, 1, 3, 17, 4096}, ns[] = {1, 5, 16}, fs[] = {0, 1, 3, 16}, ds[] = {0, 1, 3, 64};
    for (int m : ms)
        for (int n : ns)
            for (int f : fs)
                for (int depth : ds) {
                    if (f + depth < 1) continue;
                    if (m == 4096 && n == 16 && f == 16 && depth == 64) { // the largest block: its size alone
                        const ExplainLayout l = ex_layout(m, n, f, depth, EX_FIRST | EX_WALK);
                        const size_t mn = (size_t)m * n;
                        CHECK(l.copy_bytes == mn * (8 + 4 + 4 + 4) + 8 * (size_t)m + mn * f * 16 + mn * (depth + 1) * 12 + mn * depth * 8, "the largest block");
                        continue;
                    }
                    if (m > 17) continue;
                    for (uint32_t which = 0; which < (1u << 12); which += (m > 1 ? 37 : 1)) layout_of(m, n, f, depth, which);
                    layout_of(m, n, f, depth, EX_FIRST | EX_WALK);
                }
}

static void memo_and_grid() {
    const uint32_t all = EX_FIRST | EX_WALK;
    CHECK(ex_memo_on(100, 10, 16, all, 1) && !ex_memo_on(100, 10, 16, all, 0), "the hook forces it");
    CHECK(!ex_memo_on(100, 10, 0, all, 1) && !ex_memo_on(100, 10, 16, EX_FIRST, 1) && !ex_memo_on(0, 10, 16, all, 1), "no path: no memo");
    for (int m : {1, 16, 1024, 4096})
        for (int n : {1, 10, 16}) {
            const bool on = ex_memo_on(m, n, 16, all, -1);
            CHECK(on == (EX_MEMO_MIN_PAIRS >= 0 && (long long)m * n >= EX_MEMO_MIN_PAIRS), "the plan's choice at m %d n %d", m, n);
        }
    CHECK(ex_memo_elems(0, 16) == 16 && ex_memo_elems(1000, 10) == 10000 && ex_memo_elems((size_t)1 << 23, 16) == (size_t)1 << 27, "one word per (live row, lane)");
    CHECK(EX_MEMO_UNKNOWN != (((unsigned long long)(unsigned)-1 << 32) | 0u), "an empty order is not `unknown`");
    for (int m : {0, 1, 3, 4, 5, 4096})
        for (int n : {1, 5, 16}) {
            const long long pairs = (long long)m * n, waves = (long long)ex_grid(m, n) * EX_PAIR_WAVES;
            CHECK(waves >= pairs && waves - pairs < EX_PAIR_WAVES + (pairs == 0 ? 1 : 0) && ex_grid(m, n) >= 1, "one wave per pair at m %d n %d", m, n);
        }
    CHECK(EX_BLOCK == 64 * EX_PAIR_WAVES && EX_WAVE_ROWS == 64, "wave64");
}

int main() {
    arguments();
    which_bits();
    layouts();
    memo_and_grid();
    std::printf("explain_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
