// cluster_plan_test.cpp -- dynamicppr_amd/csrc/dppr_cluster_plan.hpp on the CPU: the argument check at every limit, the rank
// table's row widths, the chunk count and the bound on the chunk list against a count over random row lengths, the chunk items'
// fields, the block's sections (aligned, disjoint, inside the block, the copy ending with the last section asked for) for every
// combination of NULLs, and cluster_best against a hand-computed order, its tie rule, min_size and the prefixes it must skip; the
// arrays it reads are exactly L long (the sanitizers watch the bounds).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_cluster_plan.hpp"

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
    dppr_cluster_t b;
    CHECK(cluster_args_ok(1, 0.0, 1, &b) && cluster_args_ok(DPPR_CLUSTER_MAX, 1e-6, DPPR_CLUSTER_MAX, &b), "the limits themselves");
    CHECK(!cluster_args_ok(0, 0.0, 1, &b) && !cluster_args_ok(-1, 0.0, 1, &b) && !cluster_args_ok(DPPR_CLUSTER_MAX + 1, 0.0, 1, &b), "k");
    CHECK(!cluster_args_ok(8, -1e-300, 1, &b) && !cluster_args_ok(8, std::nan(""), 1, &b) && cluster_args_ok(8, -0.0, 1, &b), "min_p");
    CHECK(!cluster_args_ok(8, 0.0, 0, &b) && !cluster_args_ok(8, 0.0, -3, &b) && !cluster_args_ok(8, 0.0, 9, &b) && cluster_args_ok(8, 0.0, 8, &b),
          "min_size");
    CHECK(!cluster_args_ok(8, 0.0, 1, nullptr), "out_best");
    CHECK(DPPR_CLUSTER_MAX == 8192 && DPPR_CLUSTER_MAX < CL_ABSENT && CL_PER_THREAD * CL_SCAN_BLOCK == DPPR_CLUSTER_MAX, "constants");
}

static void sizes() {
    for (int n = 1; n <= Q_LANES; ++n) {
        const int s = cl_stride(n);
        CHECK(s >= n && (s & (s - 1)) == 0 && (n == 1 || s < 2 * n), "stride of %d lanes: %d", n, s);
        CHECK(cl_rank_elems(0, n) == (size_t)s && cl_rank_elems(1000, n) == (size_t)1000 * s, "rank elements, %d lanes", n);
    }
    CHECK(cl_chunks(CL_SPLIT + 1) == 2 && cl_chunks(2 * CL_SPLIT) == 2 && cl_chunks(2 * CL_SPLIT + 1) == 3, "chunks");
    // rows of random lengths that sum to Ed, both directions, every lane: the chunks of the split ones fit the list
    uint64_t x = 88172645463325252ull;
    for (int round = 0; round < 200; ++round) {
        long long Ed = 0, chunks = 0;
        const int rows = 1 + round % 37;
        for (int r = 0; r < rows; ++r) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const long long len = (long long)(x % (round % 3 == 0 ? 3 * CL_SPLIT : 40 * CL_SPLIT));
            Ed += len;
            if (len > CL_SPLIT) chunks += cl_chunks(len);
        }
        for (int n : {1, 3, 16}) CHECK((size_t)(2 * n * chunks) <= cl_list_cap(n, Ed), "round %d: %lld chunks, Ed %lld", round, chunks, Ed);
    }
    CHECK(cl_list_cap(16, 0) >= 1 && cl_list_cap(16, 2147483647ll) < ((size_t)1 << 32), "the list's limits");
    const unsigned long long it = cl_item(16u * 8192u - 1u, 1u, (1u << 20) + 5u);
    CHECK(cl_item_pos(it) == 16u * 8192u - 1u && cl_item_dir(it) == 1u && cl_item_chunk(it) == (1u << 20) + 5u, "item fields");
    CHECK(cl_item_dir(cl_item(7u, 0u, 0x7fffffffu)) == 0u && cl_item_chunk(cl_item(7u, 0u, 0x7fffffffu)) == 0x7fffffffu, "item fields, widest chunk");
}

static void layout() {
    for (int n : {1, 3, 16})
        for (int k : {1, 2, 63, 8192})
            for (int mask = 0; mask < 16; ++mask) {
                const bool ids = mask & 1, co = mask & 2, ci = mask & 4, vol = mask & 8;
                const ClLayout l = cl_layout(n, k, ids, co, ci, vol);
                const size_t nk = (size_t)n * (size_t)k;
                CHECK(l.off_best == 0 && l.off_ids == sizeof(dppr_cluster_t) * 16, "records first");
                CHECK(l.off_ids + 4 * nk <= l.off_cut_out && l.off_cut_out + 8 * nk == l.off_cut_in && l.off_cut_in + 8 * nk == l.off_vol &&
                          l.off_vol + 8 * nk == l.total_bytes,
                      "sections in order, n %d k %d", n, k);
                CHECK(l.off_cut_out % 8 == 0 && l.off_ids % 8 == 0, "alignment");
                const size_t want = vol ? l.total_bytes : ci ? l.off_vol : co ? l.off_cut_in : ids ? l.off_cut_out : l.off_ids;
                CHECK(l.copy_bytes == want && l.copy_bytes <= l.total_bytes && l.copy_bytes >= sizeof(dppr_cluster_t) * (size_t)n, "copy, mask %d", mask);
            }
    CHECK(cl_layout(16, 8192, true, true, true, true).total_bytes == 512 + (size_t)28 * 16 * 8192, "the largest block");
}

static void best_prefix() {
    const double inf = std::numeric_limits<double>::infinity();
    // Ed = 20. vol 3 8 10 12 17 20; den 3 8 10 8 3 0; cut 3 2 5 2 1 0; phi 1, .25, .5, .25, 1/3, -
    const std::vector<int64_t> cut = {3, 2, 5, 2, 1, 0}, vol = {3, 8, 10, 12, 17, 20};
    dppr_cluster_t b = cluster_best(cut.data(), vol.data(), 6, 20, 1);
    CHECK(b.count == 6 && b.best_size == 2 && b.best_cut == 2 && b.best_vol == 8 && b.best_phi == 0.25, "the first of two equal minima: %d", b.best_size);
    b = cluster_best(cut.data(), vol.data(), 6, 20, 3);
    CHECK(b.best_size == 4 && b.best_cut == 2 && b.best_vol == 12 && b.best_phi == 0.25, "min_size 3: %d", b.best_size);
    b = cluster_best(cut.data(), vol.data(), 6, 20, 5);
    CHECK(b.best_size == 5 && b.best_phi == 1.0 / 3.0, "min_size 5: %d", b.best_size);
    b = cluster_best(cut.data(), vol.data(), 6, 20, 6);
    CHECK(b.count == 6 && b.best_size == 0 && b.best_cut == 0 && b.best_vol == 0 && b.best_phi == inf, "the whole graph is not a cut");
    // a shorter order reads a shorter array
    const std::vector<int64_t> cut1 = {3}, vol1 = {3};
    b = cluster_best(cut1.data(), vol1.data(), 1, 20, 1);
    CHECK(b.count == 1 && b.best_size == 1 && b.best_phi == 1.0, "one vertex");
    // vertices of degree 0 in front: den = 0 is not eligible; a cut of 0 is the best there is
    const std::vector<int64_t> cut2 = {0, 0, 4, 0}, vol2 = {0, 0, 4, 9};
    b = cluster_best(cut2.data(), vol2.data(), 4, 20, 1);
    CHECK(b.best_size == 4 && b.best_cut == 0 && b.best_vol == 9 && b.best_phi == 0.0, "den 0 skipped: %d", b.best_size);
    b = cluster_best(nullptr, nullptr, 0, 20, 1);
    CHECK(b.count == 0 && b.best_size == 0 && b.best_phi == inf, "an empty order");
    b = cluster_best(cut2.data(), vol2.data(), 2, 0, 1);
    CHECK(b.count == 2 && b.best_size == 0 && b.best_phi == inf, "a graph without edges");
    // the division is one IEEE division: 3 / 489
    const std::vector<int64_t> cut3 = {3}, vol3 = {489};
    b = cluster_best(cut3.data(), vol3.data(), 1, 1492, 1);
    CHECK(b.best_phi == 3.0 / 489.0, "3 / 489");
}

int main() {
    arguments();
    sizes();
    layout();
    best_prefix();
    std::printf("cluster_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
