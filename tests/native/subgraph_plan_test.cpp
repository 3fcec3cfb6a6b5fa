// subgraph_plan_test.cpp -- dynamicppr_amd/csrc/dppr_subgraph_plan.hpp on the CPU: the argument check at every limit, the clamp of
// cap, the sizes, the block's sections (aligned, disjoint, inside the block, the copy running from the first to the last section
// asked for) for every combination of NULLs, which kernel fills a row, sg_slot as a stable placement, and subgraph_row against a
// hand-computed multigraph and against a sort on random rows; the arrays it reads and writes are exactly as long as it may touch
// (the sanitizers watch the bounds).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_subgraph_plan.hpp"

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
    int64_t off[2];
    int32_t cnt[1], col[1];
    CHECK(subgraph_args_ok(1, 0.0, 0, DPPR_DEST_HOST, off, cnt, nullptr) && subgraph_args_ok(DPPR_SUBGRAPH_MAX, 1e-6, 1, DPPR_DEST_DEVICE, off, cnt, col),
          "the limits themselves");
    CHECK(!subgraph_args_ok(0, 0.0, 0, 0, off, cnt, nullptr) && !subgraph_args_ok(-1, 0.0, 0, 0, off, cnt, nullptr) &&
              !subgraph_args_ok(DPPR_SUBGRAPH_MAX + 1, 0.0, 0, 0, off, cnt, nullptr),
          "k");
    CHECK(!subgraph_args_ok(8, -1e-300, 0, 0, off, cnt, nullptr) && !subgraph_args_ok(8, std::nan(""), 0, 0, off, cnt, nullptr) &&
              subgraph_args_ok(8, -0.0, 0, 0, off, cnt, nullptr),
          "min_p");
    CHECK(!subgraph_args_ok(8, 0.0, -1, 0, off, cnt, col) && !subgraph_args_ok(8, 0.0, 1, 0, off, cnt, nullptr) && subgraph_args_ok(8, 0.0, 0, 0, off, cnt, col),
          "cap and col");
    CHECK(!subgraph_args_ok(8, 0.0, 0, 2, off, cnt, nullptr) && !subgraph_args_ok(8, 0.0, 0, -1, off, cnt, nullptr), "dest");
    CHECK(!subgraph_args_ok(8, 0.0, 0, 0, nullptr, cnt, nullptr) && !subgraph_args_ok(8, 0.0, 0, 0, off, nullptr, nullptr), "offsets / counts");
    CHECK(DPPR_SUBGRAPH_MAX == 8192 && SG_PER_THREAD * SG_LONG_BLOCK == DPPR_SUBGRAPH_MAX && SG_WAVE_MAX <= SG_WAVE_CAP, "constants");
    CHECK(sg_wave_max_ok(0) && sg_wave_max_ok(SG_WAVE_CAP) && !sg_wave_max_ok(-1) && !sg_wave_max_ok(SG_WAVE_CAP + 1), "wave_max");
}

static void sizes() {
    CHECK(sg_cap_clamped(5, 100, 3) == 5 && sg_cap_clamped(300, 100, 3) == 300 && sg_cap_clamped(301, 100, 3) == 300 && sg_cap_clamped(7, 0, 16) == 0,
          "the clamp of cap");
    CHECK(sg_cap_clamped((int64_t)1 << 62, 2147483647ll, 16) == 16 * 2147483647ll, "the clamp at the largest graph");
    CHECK(sg_work_elems(16, 8192) * sizeof(int) == 16 + 2 * 16 * 8192 * 4, "the per-position work");
    CHECK(sg_ids_bytes(3, 5) == 60 && sg_p_bytes(3, 5) == 120 && sg_row_ptr_bytes(3, 5) == 144 && sg_col_bytes(7) == 28 && sg_col_bytes(-1) == 0, "sections");
    CHECK(!sg_row_is_long(CL_SPLIT, 64, 64) && sg_row_is_long(CL_SPLIT + 1, 1, 64) && sg_row_is_long(100, 65, 64) && sg_row_is_long(1, 1, 0), "which kernel");
}

static void layout() {
    for (int n : {1, 3, 16})
        for (int k : {1, 2, 63, 8192})
            for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)1001})
                for (int mask = 0; mask < 16; ++mask) {
                    const bool ids = mask & 1, p = mask & 2, rp = mask & 4, col = mask & 8;
                    const SgLayout l = sg_layout(n, k, cap, ids, p, rp, col);
                    const size_t nk = (size_t)n * (size_t)k;
                    CHECK(l.off_head == 0 && l.off_ids == SG_HEAD_BYTES && l.off_ids % 8 == 0, "the head first");
                    CHECK(l.off_ids + 4 * nk <= l.off_p && l.off_p + 8 * nk == l.off_row_ptr && l.off_row_ptr + 8 * (nk + n) == l.off_col &&
                              l.off_col + 4 * (size_t)cap <= l.total_bytes && l.total_bytes < l.off_col + 4 * (size_t)cap + 8,
                          "sections in order, n %d k %d", n, k);
                    CHECK(l.off_p % 8 == 0 && l.off_row_ptr % 8 == 0 && l.off_col % 8 == 0 && l.total_bytes % 8 == 0, "alignment");
                    const bool c = col && cap > 0;
                    const size_t lo = ids ? l.off_ids : p ? l.off_p : rp ? l.off_row_ptr : c ? l.off_col : l.total_bytes;
                    const size_t hi = c ? l.off_col + 4 * (size_t)cap : rp ? l.off_col : p ? l.off_row_ptr : ids ? l.off_p : l.total_bytes;
                    CHECK(l.copy_lo == lo && l.copy_hi == std::max(lo, hi) && l.copy_hi <= l.total_bytes, "copy, mask %d", mask);
                    CHECK((ids || p || rp || c) == (l.copy_hi > l.copy_lo), "nothing asked for, nothing copied: mask %d", mask);
                }
    CHECK(sg_layout(16, 8192, 0, true, true, true, false).total_bytes == SG_HEAD_BYTES + (size_t)20 * 16 * 8192 + 8 * 16, "the largest block without col");
}

static void row_rule() {
    // six vertices; order 1, 0, 2, 3 (positions 0..3). Row of vertex 1: heads 0, 2 -> positions 1, 2. Row of 0: heads 1, 1 -> 0, 0.
    // Row of 2: heads 2 (self loop), 3 -> 2, 3. Row of 3: heads 0, 4 -> 1 (4 lies outside the order).
    const std::vector<int32_t> pos = {1, 0, 2, 3, -1, -1};
    struct Case { std::vector<int32_t> heads, want; };
    const std::vector<Case> cases = {{{2, 0}, {1, 2}}, {{1, 1}, {0, 0}}, {{3, 2}, {2, 3}}, {{4, 0}, {1}}, {{5, 4}, {}}, {{}, {}}};
    for (const Case &c : cases) {
        std::vector<int32_t> out(c.want.size());
        const int64_t m = subgraph_row(c.heads.data(), (int64_t)c.heads.size(), pos.data(), 4, out.data());
        CHECK(m == (int64_t)c.want.size() && out == c.want, "a row of %zu entries: %lld", c.heads.size(), (long long)m);
    }
    // a shorter order: position 3 is not part of it any more
    std::vector<int32_t> pos3 = pos, out(1);
    pos3[3] = -1;
    const std::vector<int32_t> heads = {3, 2};
    CHECK(subgraph_row(heads.data(), 2, pos3.data(), 3, out.data()) == 1 && out[0] == 2, "the prefix property");
    // random rows with duplicates against a sort; sg_slot places the matched entries where the sort puts them
    uint64_t x = 88172645463325252ull;
    for (int round = 0; round < 200; ++round) {
        const int V = 5 + round % 60, L = 1 + round % V, len = round % 97;
        std::vector<int32_t> p(V, -1), hs(len), key;
        for (int j = 0; j < L; ++j) p[(j * 7 + round) % V] = -2;
        int32_t next = 0;
        for (int v = 0; v < V && next < L; ++v)
            if (p[v] == -2) p[v] = next++;
        for (int v = 0; v < V; ++v)
            if (p[v] == -2) p[v] = -1;
        for (int e = 0; e < len; ++e) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            hs[e] = (int32_t)(x % (uint64_t)V);
            if (p[hs[e]] >= 0) key.push_back(p[hs[e]]);
        }
        std::vector<int32_t> want = key, got(key.size()), placed(key.size(), -1);
        std::sort(want.begin(), want.end());
        const int64_t m = subgraph_row(hs.data(), len, p.data(), next, got.data());
        CHECK(m == (int64_t)want.size() && got == want, "round %d", round);
        std::vector<char> taken(key.size(), 0);
        for (int t = 0; t < (int)key.size(); ++t) {
            const int s = sg_slot(key.data(), (int)key.size(), t);
            CHECK(s >= 0 && s < (int)key.size() && !taken[s], "round %d: slot %d of entry %d", round, s, t);
            if (s >= 0 && s < (int)key.size()) taken[s] = 1, placed[s] = key[t];
        }
        CHECK(placed == want, "round %d: the slots are the sort", round);
    }
}

int main() {
    arguments();
    sizes();
    layout();
    row_rule();
    std::printf("subgraph_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
