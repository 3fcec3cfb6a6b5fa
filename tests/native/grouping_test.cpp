// CPU test driver for dynamicppr_amd/csrc/dppr_grouping.hpp (which implementation groups a batch's records by tail): the bucket
// count steps where the bucket path's lengths say, the fullest bucket equals a plain count on random and skewed tails, and the path
// selection at every boundary (length, fullest bucket, the radix switch).   grouping_test <seed> <cases>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

#include "../../dynamicppr_amd/csrc/dppr_grouping.hpp"

using namespace dppr;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 10) { printf("FAILED %s (line %d): ", #c, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    const int cases = argc > 2 ? atoi(argv[2]) : 200;
    std::mt19937 rng(seed);
    // nb: 64 up to 32 768 records, doubling one record after every further power of two, 4 096 from 2 Mi + 1 on
    CHECK(grouping_buckets(1) == 64 && grouping_buckets(4097) == 64 && grouping_buckets(32768) == 64, "small");
    for (int nb = 128, L = 32768; nb <= SU_GRP_MAX_BUCKETS; nb *= 2, L *= 2) {
        CHECK(grouping_buckets(L) == nb / 2, "L %d", L);
        CHECK(grouping_buckets(L + 1) == nb, "L %d", L + 1);
    }
    CHECK(grouping_buckets(SU_GRP_MAX_RECORDS) == SU_GRP_MAX_BUCKETS && grouping_buckets(SU_GRP_MAX_RECORDS + 1) == SU_GRP_MAX_BUCKETS, "cap");
    // the path by length alone
    CHECK(grouping_path(SU_RANK_MAX, 0, false) == GROUPING_RANK, "rank");
    CHECK(grouping_path(SU_RANK_MAX + 1, 1, false) == GROUPING_BUCKET, "bucket");
    CHECK(grouping_path(SU_GRP_MAX_RECORDS, SU_GRP_MAX_BUCKET, false) == GROUPING_BUCKET, "bucket at the cap");
    CHECK(grouping_path(SU_GRP_MAX_RECORDS, SU_GRP_MAX_BUCKET + 1, false) == GROUPING_RADIX, "hot bucket");
    CHECK(grouping_path(SU_GRP_MAX_RECORDS + 1, 0, false) == GROUPING_RADIX, "length");
    CHECK(grouping_path(1, 0, true) == GROUPING_RADIX && grouping_path(100000, 10, true) == GROUPING_RADIX, "switch");
    // the fullest bucket against a plain count, on batches of all shapes around the boundaries
    const int lengths[] = {1, 4096, 4097, 32768, 32769, 65537, 262145, 1 << 20, (1 << 20) + 1};
    long long checked = 0;
    for (int c = 0; c < cases && fails == 0; ++c) {
        const int L = lengths[rng() % (sizeof(lengths) / sizeof(lengths[0]))];
        const int V = 1 + (int)(rng() % (1u << (1 + rng() % 24)));
        const double hot = (rng() % 3 == 0) ? 0.0 : (rng() % 1000) / 1000.0;
        const int hub = (int)(rng() % (unsigned)V);
        std::vector<int32_t> t((size_t)L);
        for (auto &x : t) x = (rng() % 1000) < hot * 1000 ? hub : (int32_t)(rng() % (unsigned)V);
        const int got = largest_bucket(t.data(), L);
        if (L <= SU_RANK_MAX || L > SU_GRP_MAX_RECORDS) {
            CHECK(got == 0, "L %d: %d", L, got);
            continue;
        }
        const int nb = grouping_buckets(L);
        std::map<int, int> h;
        int want = 0;
        for (int x : t) want = std::max(want, ++h[x % nb]);
        CHECK(got == want, "L %d V %d hot %.3f: %d, plain count %d", L, V, hot, got, want);
        const GroupingPath p = grouping_path(L, got, false);
        CHECK(p == (want > SU_GRP_MAX_BUCKET ? GROUPING_RADIX : GROUPING_BUCKET), "L %d fullest %d: path %d", L, want, (int)p);
        ++checked;
    }
    printf("grouping_test seed %u: %lld batches counted, %d failures\n", seed, checked, fails);
    return fails ? 1 : 0;
}
