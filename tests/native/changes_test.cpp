// changes_test.cpp -- dynamicppr_amd/csrc/dppr_changes_plan.hpp on the CPU: the result block of dppr_changes /
// dppr_group_changes for every lane count and a spread of k (sections aligned, in the documented order, disjoint, inside the
// block, the copied part a prefix), a block written section by section into a buffer of exactly total_bytes (the sanitizers
// watch the bounds), and the argument check against a plain restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_changes_plan.hpp"

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

int main() {
    long cases = 0;
    const int ks[] = {1, 2, 3, 7, 8, 9, 10, 255, 256, 257, 1000, 4095, 4096, 8191, 8192};
    for (int n = 1; n <= CH_LANES; ++n)
        for (int k : ks) {
            const ChLayout l = ch_layout(n, k);
            const size_t nk = (size_t)n * (size_t)k;
            ++cases;
            CHECK(l.off_cnt == 0 && l.off_moved == 64 && l.off_ids == 128, "n %d k %d", n, k);
            CHECK(l.off_delta >= l.off_ids + sizeof(int) * nk && l.off_delta < l.off_ids + sizeof(int) * nk + 8, "n %d k %d", n, k);
            CHECK(l.off_delta % 8 == 0 && l.off_p % 8 == 0 && l.off_abs % 8 == 0, "n %d k %d", n, k);
            CHECK(l.off_p == l.off_delta + 8 * nk && l.off_abs == l.off_p + 8 * nk, "n %d k %d", n, k);
            CHECK(l.copy_bytes == l.off_abs && l.total_bytes == l.off_abs + 8 * nk, "n %d k %d", n, k);
            const ChLayout top = ch_layout(CH_LANES, CH_K_MAX);
            CHECK(l.total_bytes <= top.total_bytes && l.copy_bytes <= top.copy_bytes, "n %d k %d", n, k);
            // every section written whole into a block of exactly total_bytes, then read back: no two overlap
            std::vector<unsigned char> block(l.total_bytes, 0xEE);
            std::vector<int32_t> cnt((size_t)CH_LANES, 1), moved((size_t)CH_LANES, 2), ids(nk, 3);
            std::vector<double> d(nk, 4.0), p(nk, 5.0), a(nk, 6.0);
            std::memcpy(block.data() + l.off_cnt, cnt.data(), 4 * (size_t)CH_LANES);
            std::memcpy(block.data() + l.off_moved, moved.data(), 4 * (size_t)CH_LANES);
            std::memcpy(block.data() + l.off_ids, ids.data(), 4 * nk);
            std::memcpy(block.data() + l.off_delta, d.data(), 8 * nk);
            std::memcpy(block.data() + l.off_p, p.data(), 8 * nk);
            std::memcpy(block.data() + l.off_abs, a.data(), 8 * nk);
            std::vector<int32_t> i2(nk);
            std::vector<double> d2(nk), p2(nk), a2(nk);
            int32_t c2[CH_LANES], m2[CH_LANES];
            std::memcpy(c2, block.data() + l.off_cnt, sizeof(c2));
            std::memcpy(m2, block.data() + l.off_moved, sizeof(m2));
            std::memcpy(i2.data(), block.data() + l.off_ids, 4 * nk);
            std::memcpy(d2.data(), block.data() + l.off_delta, 8 * nk);
            std::memcpy(p2.data(), block.data() + l.off_p, 8 * nk);
            std::memcpy(a2.data(), block.data() + l.off_abs, 8 * nk);
            bool same = i2 == ids && d2 == d && p2 == p && a2 == a;
            for (int s = 0; s < CH_LANES; ++s) same = same && c2[s] == 1 && m2[s] == 2;
            CHECK(same, "sections overlap: n %d k %d", n, k);
        }
    // the argument check
    int x = 0;
    const void *some = &x;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int kk[] = {-1, 0, 1, 2, CH_K_MAX - 1, CH_K_MAX, CH_K_MAX + 1, 1 << 30};
    const double mm[] = {-inf, -1.0, -1e-300, -0.0, 0.0, 1e-300, 1e-12, 1.0, inf, nan};
    for (int k : kk)
        for (double m : mm)
            for (int mask = 0; mask < 8; ++mask) {
                ++cases;
                const void *a = mask & 1 ? some : nullptr, *b = mask & 2 ? some : nullptr, *c = mask & 4 ? some : nullptr;
                const bool want = k >= 1 && k <= 8192 && !std::isnan(m) && !(m < 0.0) && mask == 7;
                CHECK(ch_args_ok(k, m, a, b, c) == want, "k %d m %g mask %d", k, m, mask);
            }
    std::printf("changes_test: %ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
