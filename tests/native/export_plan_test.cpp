// export_plan_test.cpp -- dynamicppr_amd/csrc/dppr_export_plan.hpp on the CPU: tile counts, the workspace, the block of a sparse
// export (sections aligned, in order, disjoint, inside the block; written whole into a buffer of exactly total_bytes: the
// sanitizers watch the bounds), the bytes, alignment and indices of a dense destination for every (dtype, layout, n, V), 64-bit
// arithmetic where V * n passes 2^31, the range check of a destination and the argument checks against plain restatements.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_export_plan.hpp"

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
    const int64_t Vs[] = {1, 255, 256, 257, (int64_t)1 << 22};
    // tiles and workspace
    for (int64_t V : Vs) {
        ++cases;
        int64_t want = 0;
        for (int64_t v = 0; v < V; v += EX_TILE) ++want;
        CHECK(ex_tiles(V) == want, "V %lld", (long long)V);
        const ExWork w = ex_workspace(V);
        CHECK(w.mask_elems == (size_t)V && w.cnt_elems == (size_t)want * 16 && w.base_elems == (size_t)want * 16, "V %lld", (long long)V);
        CHECK(w.bytes == 2 * (size_t)V + 192 * (size_t)want, "V %lld", (long long)V);
    }
    CHECK(ex_tiles((int64_t)1 << 22) == 16384, "16 Ki tiles at 2^22 ids");
    CHECK(ex_tiles(((int64_t)1 << 31) + 5) == ((int64_t)1 << 23) + 1, "tile count past 2^31 ids");
    static_assert(EX_TILE <= 256 && EX_TILE % 64 == 0, "a tile is whole waves, at most 256 ids");
    static_assert(EX_HEAD_BYTES % 8 == 0, "the sections start aligned");
    // dense destinations
    for (int dtype : {DPPR_F64, DPPR_F32})
        for (int layout : {DPPR_VERTEX_MAJOR, DPPR_SOURCE_MAJOR})
            for (int n = 1; n <= EX_LANES; ++n)
                for (int64_t V : Vs) {
                    ++cases;
                    const size_t el = dtype == DPPR_F32 ? 4 : 8;
                    CHECK(ex_elem_bytes(dtype) == el, "dtype %d", dtype);
                    const size_t bytes = ex_dense_bytes(dtype, n, V);
                    CHECK(bytes == el * (uint64_t)n * (uint64_t)V, "dtype %d n %d V %lld", dtype, n, (long long)V);
                    // corners: first and last element, and the neighbours in both directions are distinct and inside
                    const size_t first = ex_dense_index(layout, n, V, 0, 0), last = ex_dense_index(layout, n, V, V - 1, n - 1);
                    CHECK(first == 0 && last == (size_t)n * (size_t)V - 1, "dtype %d layout %d n %d V %lld", dtype, layout, n, (long long)V);
                    CHECK((last + 1) * el == bytes, "the last element ends the destination");
                    if (V > 1) {
                        const size_t a = ex_dense_index(layout, n, V, 1, 0);
                        CHECK(a == (layout == DPPR_SOURCE_MAJOR ? (size_t)1 : (size_t)n), "vertex stride");
                    }
                    if (n > 1) {
                        const size_t a = ex_dense_index(layout, n, V, 0, 1);
                        CHECK(a == (layout == DPPR_SOURCE_MAJOR ? (size_t)V : (size_t)1), "source stride");
                    }
                    if (V <= 257) { // every (v, i) once
                        std::vector<unsigned char> seen((size_t)n * (size_t)V, 0);
                        for (int64_t v = 0; v < V; ++v)
                            for (int i = 0; i < n; ++i) seen[ex_dense_index(layout, n, V, v, i)]++;
                        bool once = true;
                        for (unsigned char c : seen) once = once && c == 1;
                        CHECK(once, "a bijection: layout %d n %d V %lld", layout, n, (long long)V);
                    }
                }
    // 64-bit: V * n beyond 2^31
    {
        ++cases;
        const int64_t V = ((int64_t)1 << 28) + 3;
        CHECK(ex_dense_bytes(DPPR_F64, 16, V) == (size_t)8 * 16 * (size_t)V, "bytes past 2^35");
        CHECK(ex_dense_index(DPPR_SOURCE_MAJOR, 16, V, V - 1, 15) == (size_t)16 * (size_t)V - 1, "index past 2^31");
        CHECK(ex_dense_index(DPPR_VERTEX_MAJOR, 16, V, V - 1, 15) == (size_t)16 * (size_t)V - 1, "index past 2^31");
        CHECK(ex_cap_clamped(std::numeric_limits<int64_t>::max(), V, 16) == 16 * V, "cap clamps to V * n in 64 bits");
        CHECK(ex_cap_clamped(5, V, 16) == 5, "a small cap stays");
        const ExLayout l = ex_layout(16 * V, true);
        CHECK(l.off_p == EX_HEAD_BYTES + 4 * (size_t)16 * (size_t)V + 0 + ((4 * (size_t)16 * (size_t)V) % 8 ? 4 : 0), "ids section past 2^32 bytes");
        CHECK(l.total_bytes == l.off_p + 2 * 8 * (size_t)16 * (size_t)V, "block past 2^36 bytes");
    }
    // the block of a sparse export
    const int64_t caps[] = {0, 1, 2, 3, 7, 8, 255, 256, 257, 100003};
    for (int64_t cap : caps)
        for (int with_r = 0; with_r < 2; ++with_r) {
            ++cases;
            const ExLayout l = ex_layout(cap, with_r != 0);
            const size_t c = (size_t)cap;
            CHECK(l.off_ids == EX_HEAD_BYTES && l.off_ids == 144, "cap %lld", (long long)cap);
            CHECK(l.off_p >= l.off_ids + 4 * c && l.off_p < l.off_ids + 4 * c + 8 && l.off_p % 8 == 0, "cap %lld", (long long)cap);
            CHECK(l.off_r == l.off_p + 8 * c && l.total_bytes == l.off_r + (with_r ? 8 * c : 0), "cap %lld", (long long)cap);
            std::vector<unsigned char> block(l.total_bytes, 0xEE);
            ExHead head;
            for (int i = 0; i <= EX_LANES; ++i) head.offsets[i] = 1000 + i;
            head.go = 1;
            head.pad = 0;
            std::vector<int32_t> ids(c, 3);
            std::vector<double> p(c, 5.0), r(c, 6.0);
            std::memcpy(block.data(), &head, sizeof(head));
            if (c) std::memcpy(block.data() + l.off_ids, ids.data(), 4 * c);
            if (c) std::memcpy(block.data() + l.off_p, p.data(), 8 * c);
            if (c && with_r) std::memcpy(block.data() + l.off_r, r.data(), 8 * c);
            ExHead h2;
            std::vector<int32_t> i2(c);
            std::vector<double> p2(c), r2(c, 6.0);
            std::memcpy(&h2, block.data(), sizeof(h2));
            if (c) std::memcpy(i2.data(), block.data() + l.off_ids, 4 * c);
            if (c) std::memcpy(p2.data(), block.data() + l.off_p, 8 * c);
            if (c && with_r) std::memcpy(r2.data(), block.data() + l.off_r, 8 * c);
            bool same = i2 == ids && p2 == p && r2 == r && h2.go == 1;
            for (int i = 0; i <= EX_LANES; ++i) same = same && h2.offsets[i] == 1000 + i;
            CHECK(same, "sections overlap: cap %lld with_r %d", (long long)cap, with_r);
        }
    CHECK(ex_layout(-5, true).total_bytes == EX_HEAD_BYTES, "a negative cap is the head alone");
    // the range check of a destination
    {
        const uintptr_t base = 0x10000;
        const size_t size = 4096;
        struct { uintptr_t ptr; size_t bytes, align; bool want; } rs[] = {
            {base, 4096, 8, true}, {base, 4097, 8, false}, {base + 8, 4088, 8, true}, {base + 8, 4089, 8, false},
            {base + 4, 8, 8, false}, {base + 4, 8, 4, true}, {base + 2, 4, 4, false}, {base - 8, 8, 8, false}, {0, 0, 8, false},
            {base + 4096, 0, 8, true}, {base + 4096, 1, 8, false}, {base + 4104, 0, 8, false},
            {base, std::numeric_limits<size_t>::max(), 8, false}, {base + 8, std::numeric_limits<size_t>::max() - 4, 8, false}};
        for (auto &c : rs) {
            ++cases;
            CHECK(ex_range_ok(c.ptr, c.bytes, c.align, base, size) == c.want, "ptr %#lx bytes %zu align %zu", (unsigned long)c.ptr, c.bytes, c.align);
        }
    }
    // the argument checks
    int x = 0;
    const void *some = &x;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double mm[] = {-inf, -1.0, -1e-300, -0.0, 0.0, 1e-300, 1e-9, 1.0, inf, nan};
    const int64_t cc[] = {std::numeric_limits<int64_t>::min(), -1, 0, 1, 1000, std::numeric_limits<int64_t>::max()};
    for (double m : mm)
        for (int64_t cap : cc)
            for (int dest = -1; dest <= 2; ++dest)
                for (int mask = 0; mask < 8; ++mask) {
                    ++cases;
                    const void *o = mask & 1 ? some : nullptr, *i = mask & 2 ? some : nullptr, *p = mask & 4 ? some : nullptr;
                    const bool want = !std::isnan(m) && !(m < 0.0) && cap >= 0 && (dest == 0 || dest == 1) && o && (cap == 0 || (i && p));
                    CHECK(ex_sparse_args_ok(m, cap, dest, o, i, p) == want, "m %g cap %lld dest %d mask %d", m, (long long)cap, dest, mask);
                }
    for (double m : mm) {
        ++cases;
        CHECK(ex_support_args_ok(m, some) == (!std::isnan(m) && !(m < 0.0)) && !ex_support_args_ok(m, nullptr), "m %g", m);
    }
    for (int which = -1; which <= 2; ++which)
        for (int dtype = -1; dtype <= 2; ++dtype)
            for (int layout = -1; layout <= 2; ++layout) {
                ++cases;
                const bool want = (which == 0 || which == 1) && (dtype == 0 || dtype == 1) && (layout == 0 || layout == 1);
                CHECK(ex_dense_args_ok(which, dtype, layout) == want, "which %d dtype %d layout %d", which, dtype, layout);
            }
    std::printf("export_plan_test: %ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
