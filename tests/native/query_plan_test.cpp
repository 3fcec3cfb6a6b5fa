// query_plan_test.cpp -- dynamicppr_amd/csrc/dppr_query_plan.hpp on the CPU: the result block of a top-k call (sections aligned,
// in order, inside the block; written whole into a buffer of exactly total_bytes: the sanitizers watch the bounds), the buffer of
// the point reads, the id range check and the argument checks of top-k, the point reads and the weighted forms, against plain
// restatements.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_query_plan.hpp"

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

// the next multiple of 8, restated plainly
static size_t up8(size_t x) {
    while (x % 8) ++x;
    return x;
}

int main() {
    long cases = 0;
    static_assert(Q_LANES == 16 && DPPR_TOPK_MAX == 8192 && TK_OFF_IDS == 64, "the constants of the contract");
    for (size_t x = 0; x <= 64; ++x) CHECK(pad8(x) == up8(x), "pad8(%zu)", x);
    CHECK(pad8(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 8, "pad8 past 2^32");

    // the block of a top-k call
    const int ks[] = {1, 2, 3, 100, 8191, 8192};
    for (int n = 1; n <= 16; ++n)
        for (int k : ks)
            for (int with_r = 0; with_r <= 1; ++with_r) {
                ++cases;
                const TkLayout l = tk_layout(n, k, with_r != 0);
                const size_t nk = (size_t)n * (size_t)k, ids_end = 64 + up8(4 * nk);
                CHECK(l.off_cnt == 0 && l.off_ids == 64 && l.off_ids >= 4 * (size_t)Q_LANES, "n %d k %d: counts, then ids", n, k);
                CHECK(l.off_p == ids_end && l.off_r == ids_end + 8 * nk, "n %d k %d: p, then r", n, k);
                CHECK(l.off_p % 8 == 0 && l.off_r % 8 == 0, "n %d k %d: doubles 8-aligned", n, k);
                CHECK(l.copy_bytes == ids_end + 8 * nk * (with_r ? 2 : 1), "n %d k %d r %d: copy bytes", n, k, with_r);
                CHECK(l.total_bytes == ids_end + 8 * nk * 2, "n %d k %d r %d: the device block holds r either way", n, k, with_r);
                CHECK(l.copy_bytes <= l.total_bytes && l.total_bytes <= tk_layout(16, 8192, true).total_bytes, "n %d k %d: inside the first-use block", n, k);
                // every section written whole into a block of exactly total_bytes, read back from what is copied
                std::vector<unsigned char> block(l.total_bytes, 0xee);
                std::vector<int32_t> cnt((size_t)n, 1), ids(nk, 3);
                std::vector<double> p(nk, 0.5), r(nk, -0.25);
                std::memcpy(block.data() + l.off_cnt, cnt.data(), 4 * (size_t)n);
                std::memcpy(block.data() + l.off_ids, ids.data(), 4 * nk);
                std::memcpy(block.data() + l.off_p, p.data(), 8 * nk);
                std::memcpy(block.data() + l.off_r, r.data(), 8 * nk);
                std::vector<unsigned char> pin(block.begin(), block.begin() + (long)l.copy_bytes);
                std::vector<int32_t> ids2(nk);
                std::vector<double> p2(nk), r2(nk, -0.25);
                std::memcpy(ids2.data(), pin.data() + l.off_ids, 4 * nk);
                std::memcpy(p2.data(), pin.data() + l.off_p, 8 * nk);
                if (with_r) std::memcpy(r2.data(), pin.data() + l.off_r, 8 * nk);
                CHECK(ids2 == ids && p2 == p && r2 == r, "n %d k %d r %d: the sections do not overlap", n, k, with_r);
            }
    CHECK(tk_layout(16, 8192, true).total_bytes == 64 + 524288 + 2 * 1048576, "the first-use allocation: 2621504 bytes");
    CHECK(tk_layout(1, 1, false).off_p == 72 && tk_layout(3, 3, true).off_p == 64 + 40, "n k odd: the ids are padded");

    // the buffer of the point reads: dppr_read_at (p and r, [m][n]) and dppr_group_score_at (scores, [m][q])
    const int ms[] = {1, 2, 3, 4096};
    for (int m : ms)
        for (int cols = 1; cols <= 16; ++cols) {
            ++cases;
            const size_t mc = (size_t)m * (size_t)cols;
            const RaLayout two = ra_layout(m, cols, 2), one = ra_layout(m, cols, 1);
            CHECK(two.off_ids == 0 && two.off_a == up8(4 * (size_t)m) && two.off_b == two.off_a + 8 * mc, "m %d cols %d: ids, p, r", m, cols);
            CHECK(two.off_a % 8 == 0 && two.off_b % 8 == 0, "m %d cols %d: doubles 8-aligned", m, cols);
            CHECK(two.total_bytes == up8(4 * (size_t)m) + 16 * mc, "m %d cols %d: read_at bytes", m, cols);
            CHECK(one.off_ids == 0 && one.off_a == two.off_a && one.total_bytes == up8(4 * (size_t)m) + 8 * mc, "m %d cols %d: score_at bytes", m, cols);
            std::vector<unsigned char> buf(two.total_bytes, 0);
            std::vector<int32_t> ids((size_t)m, 7);
            std::vector<double> a(mc, 1.5), b(mc, 2.5);
            std::memcpy(buf.data() + two.off_ids, ids.data(), 4 * (size_t)m);
            std::memcpy(buf.data() + two.off_a, a.data(), 8 * mc);
            std::memcpy(buf.data() + two.off_b, b.data(), 8 * mc);
            CHECK(std::memcmp(buf.data() + two.off_ids, ids.data(), 4 * (size_t)m) == 0 && std::memcmp(buf.data() + two.off_a, a.data(), 8 * mc) == 0,
                  "m %d cols %d: the sections do not overlap", m, cols);
        }

    // every id in [0, V)
    {
        const int64_t V = 10;
        const int32_t edge[] = {-1, 0, (int32_t)V - 1, (int32_t)V};
        for (int32_t id : edge) {
            ++cases;
            const int32_t ids[3] = {4, 5, id}; // (the last entry: every entry is looked at)
            CHECK(ids_in_range(ids, 3, V) == (id >= 0 && id < V), "id %d", id);
            CHECK(ids_in_range(ids, 2, V), "id %d beyond m is not read", id);
            CHECK(read_at_args_ok(ids, 3, V) == (id >= 0 && id < V), "read_at id %d", id);
        }
        CHECK(ids_in_range(nullptr, 0, V) && read_at_args_ok(nullptr, 0, V), "m = 0 reads nothing");
        const int32_t ok[2] = {0, 9};
        CHECK(!read_at_args_ok(ok, -1, V) && !read_at_args_ok(nullptr, 2, V) && read_at_args_ok(ok, 2, V) && read_at_args_ok(ok, 0, V), "m and a null ids");
        const int32_t big[1] = {std::numeric_limits<int32_t>::max()};
        CHECK(!ids_in_range(big, 1, (int64_t)std::numeric_limits<int32_t>::max()) && ids_in_range(big, 1, (int64_t)1 << 31), "V at 2^31");
    }

    // the arguments of a top-k call
    int x = 0;
    const void *some = &x;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int32_t kk[] = {std::numeric_limits<int32_t>::min(), -1, 0, 1, 8192, 8193, std::numeric_limits<int32_t>::max()};
    const double mm[] = {nan, -inf, -1.0, -0.0, 0.0, 1e-300, 1.0, inf};
    for (int32_t k : kk)
        for (double m : mm)
            for (int mask = 0; mask < 8; ++mask) {
                ++cases;
                const void *i = mask & 1 ? some : nullptr, *p = mask & 2 ? some : nullptr, *c = mask & 4 ? some : nullptr;
                const bool want = k >= 1 && k <= 8192 && !std::isnan(m) && !(m < 0.0) && i && p && c;
                CHECK(topk_args_ok(k, m, i, p, c) == want, "k %d min_p %g mask %d", k, m, mask);
            }

    // weights [q][n]
    for (int n = 1; n <= 16; n += 5)
        for (int q = -1; q <= 17; ++q) {
            ++cases;
            const size_t qn = q > 0 ? (size_t)q * (size_t)n : 0;
            std::vector<double> w(qn, 0.25); // exactly q x n entries: nothing beyond them is read
            const bool q_ok = q >= 1 && q <= 16;
            CHECK(weights_ok(w.data(), q, n) == q_ok, "q %d n %d", q, n);
            CHECK(!weights_ok(nullptr, q, n), "q %d n %d: null weights", q, n);
            if (!q_ok) continue;
            for (double bad : {nan, inf, -inf})
                for (size_t at : {(size_t)0, qn / 2, qn - 1}) {
                    std::vector<double> wb(w);
                    wb[at] = bad;
                    CHECK(!weights_ok(wb.data(), q, n), "q %d n %d: %g at %zu", q, n, bad, at);
                }
            w[qn - 1] = -1e300;
            w[0] = -0.0;
            CHECK(weights_ok(w.data(), q, n), "q %d n %d: negative and zero weights are finite", q, n);
        }
    // the scratch state of the weighted, changes and ranked queries
    ++cases;
    CHECK(scratch_plane_elems(0, 3) == 3 && scratch_plane_elems(1000, 10) == 10000 && scratch_ext_elems(0) == 1 && scratch_ext_elems(77) == 77,
          "scratch state");
    std::printf("query_plan_test: %ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
