// dot_plan_test.cpp -- dynamicppr_amd/csrc/dppr_dot_plan.hpp on the CPU: tile, block and column counts, the tile table of a sparse
// call (tiles in order, disjoint, covering every entry once, every query on a block of its own; read whole through a buffer of
// exactly the planned bytes: the sanitizers watch the bounds), 64-bit sizes beyond 2^31, the workspace sizes, the argument and
// offset checks, and dot_fold_ref against a plain recursive tree, against a crafted cancellation vector, and against the fold cut
// into the pieces the device uses (leaf counters of every group count, subtile, tile, block).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_dot_plan.hpp"

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

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}

static double add(double a, double b) {
    volatile double s = a + b;
    return s;
}

// the balanced tree over t[lo, lo + len), len a power of two, slots at or past m are +0.0
static double tree(const double *t, int64_t m, int64_t lo, int64_t len) {
    if (len == 1) return lo < m ? t[lo] : 0.0;
    return add(tree(t, m, lo, len / 2), tree(t, m, lo + len / 2, len / 2));
}

static double fold_plain(const double *t, int64_t m) {
    if (m <= 0) return 0.0;
    double acc = tree(t, m, 0, DOT_BLOCK);
    for (int64_t b = 1; b * DOT_BLOCK < m; ++b) acc = add(acc, tree(t, m, b * DOT_BLOCK, DOT_BLOCK));
    return acc;
}

// a binary counter of partial sums over steps of U terms (U = 8 where L allows, else pairs; each step a static tree): what a thread
// of the device does over L terms
static double counter_leaf(const double *t, int L) {
    if (L == 1) return t[0];
    const int U = L >= 8 ? 8 : 2;
    double lvl[16] = {0};
    double v = 0.0;
    for (int j = 0; U * j < L; ++j) {
        const double *q = t + U * j;
        v = U == 8 ? add(add(add(q[0], q[1]), add(q[2], q[3])), add(add(q[4], q[5]), add(q[6], q[7]))) : add(q[0], q[1]);
        for (int k = 0; k < 16; ++k) {
            if (!((j >> k) & 1)) {
                lvl[k] = v;
                break;
            }
            v = add(lvl[k], v);
        }
    }
    return v;
}

// the fold as the device cuts it, with G slot groups per subtile
static double fold_pieces(const double *t, int64_t m, int G) {
    if (m <= 0) return 0.0;
    const int64_t tiles = dot_tiles(m), cols = dot_cols(m);
    std::vector<double> part((size_t)cols, 0.0);
    for (int64_t tile = 0; tile < tiles; ++tile) {
        double sums[DOT_SUB];
        for (int sub = 0; sub < DOT_SUB; ++sub) {
            const int64_t e0 = tile * DOT_WG_SLOTS + (int64_t)sub * DOT_TILE;
            if (e0 >= m) {
                sums[sub] = 0.0;
                continue;
            }
            double st[DOT_TILE], grp[DOT_TILE];
            for (int j = 0; j < DOT_TILE; ++j) st[j] = e0 + j < m ? t[e0 + j] : 0.0;
            const int L = DOT_TILE / G;
            for (int g = 0; g < G; ++g) grp[g] = counter_leaf(st + g * L, L);
            for (int step = 1; step < G; step *= 2)
                for (int g = 0; g < G; g += 2 * step) grp[g] = add(grp[g], grp[g + step]);
            sums[sub] = grp[0];
        }
        part[(size_t)tile] = counter_leaf(sums, DOT_SUB);
    }
    double acc = 0.0;
    for (int64_t b = 0; b < cols / DOT_TPB; ++b) {
        double y[DOT_TPB];
        for (int j = 0; j < DOT_TPB; ++j) y[j] = part[(size_t)(b * DOT_TPB + j)];
        for (int len = DOT_TPB; len > 1; len /= 2)
            for (int j = 0; j < len / 2; ++j) y[j] = add(y[2 * j], y[2 * j + 1]);
        acc = b == 0 ? y[0] : add(acc, y[0]);
    }
    return acc;
}

int main() {
    long cases = 0;
    static_assert(DOT_TILE == 256 && DOT_WG_SLOTS == 2048 && DOT_BLOCK == 65536 && DOT_TPB == 32 && DPPR_DOT_MAX_F == 4096, "the constants of the contract");
    const int64_t Ms[] = {0, 1, 255, 256, 257, 65535, 65536, 65537, (int64_t)1 << 22};
    // tile, block and column counts
    for (int64_t m : Ms) {
        ++cases;
        int64_t tiles = 0, blocks = 0;
        for (int64_t s = 0; s < m; s += DOT_WG_SLOTS) ++tiles;
        for (int64_t s = 0; s < m; s += DOT_BLOCK) ++blocks;
        CHECK(dot_tiles(m) == tiles && dot_blocks(m) == blocks && dot_cols(m) == blocks * 32, "m %lld", (long long)m);
        CHECK(dot_cols(m) >= dot_tiles(m), "every tile has a column, m %lld", (long long)m);
    }
    CHECK(dot_tiles(((int64_t)1 << 33) + 1) == ((int64_t)1 << 22) + 1, "tile count past 2^31 slots");
    CHECK(dot_cols(((int64_t)1 << 33) + 1) == (((int64_t)1 << 17) + 1) * 32, "column count past 2^31 slots");
    CHECK(dot_dense_h_bytes(DPPR_F64, 4096, ((int64_t)1 << 31) - 1) == (size_t)8 * 4096 * (size_t)(((int64_t)1 << 31) - 1), "h bytes past 2^31");
    CHECK(dot_dense_h_bytes(DPPR_F32, 3, 1000) == 12000 && dot_elem_bytes(DPPR_F32) == 4 && dot_elem_bytes(DPPR_F64) == 8, "element sizes");
    CHECK(dot_h_index(DPPR_H_FEATURE_MAJOR, 4096, (int64_t)1 << 30, 4095, ((int64_t)1 << 30) - 1) == ((size_t)1 << 42) - 1, "last element, feature-major");
    CHECK(dot_h_index(DPPR_H_VERTEX_MAJOR, 4096, (int64_t)1 << 30, 4095, ((int64_t)1 << 30) - 1) == ((size_t)1 << 42) - 1, "last element, vertex-major");
    CHECK(dot_h_index(DPPR_H_FEATURE_MAJOR, 7, 100, 2, 5) == 205 && dot_h_index(DPPR_H_VERTEX_MAJOR, 7, 100, 2, 5) == 37, "strides");
    CHECK(dot_out_bytes(4096, 16) == 524288 && dot_block_bytes(3, 10, DPPR_DEST_HOST) == 8 + 240 && dot_block_bytes(3, 10, DPPR_DEST_DEVICE) == 8, "block");
    // the dense workspace: whole chunks inside the budget, one chunk at the least, never more features than asked for
    for (int64_t V : {(int64_t)1, (int64_t)257, (int64_t)65536 + 257, (int64_t)1 << 22, ((int64_t)1 << 31) - 1})
        for (int n : {1, 3, 10, 16})
            for (int F : {1, 15, 16, 17, 64, 4096}) {
                ++cases;
                const int lf = dot_launch_features(V, n, F);
                CHECK(lf >= 1 && lf <= F && (lf == F || lf % DOT_FCHUNK == 0), "V %lld n %d F %d: %d", (long long)V, n, F, lf);
                const size_t elems = dot_dense_part_elems(V, n, F);
                CHECK(elems == (size_t)lf * n * (size_t)dot_cols(V), "V %lld n %d F %d", (long long)V, n, F);
                CHECK(lf <= DOT_FCHUNK || 8 * elems <= DOT_PART_BUDGET, "V %lld n %d F %d: %zu bytes", (long long)V, n, F, 8 * elems);
                // the last partial a launch writes lies inside
                const size_t last = ((size_t)lf * n - 1) * (size_t)dot_cols(V) + (size_t)dot_tiles(V) - 1;
                CHECK(last < elems, "V %lld n %d F %d", (long long)V, n, F);
            }
    for (int outs = 1; outs <= 256; ++outs) {
        ++cases;
        const int G = dot_groups(outs);
        CHECK(G >= 1 && (G & (G - 1)) == 0 && G * outs <= DOT_TILE && 2 * G * outs > DOT_TILE, "outs %d G %d", outs, G);
    }
    CHECK(dot_lds_bytes(16, 16) == 8 * (256 * 17 + 16 * 257 + 256) + 1024 && dot_lds_bytes(16, 16) <= 160 * 1024 / 2, "two workgroups of the widest pass per CU");
    CHECK(dot_lds_bytes(1, 1) == 8 * (512 + 257 + 256) + 1024, "a slot");

    // the tile table
    {
        const std::vector<std::vector<int64_t>> lens = {{0}, {1}, {255}, {256}, {257}, {65535}, {65536}, {65537}, {(int64_t)1 << 22},
                                                        {0, 1, 65537}, {5, 0, 0, 2048, 2049, 0, 70000, 1}, {0, 0, 0}};
        for (const auto &ln : lens) {
            ++cases;
            const int F = (int)ln.size();
            std::vector<int64_t> off(1, 0);
            for (int64_t l : ln) off.push_back(off.back() + l);
            CHECK(dot_offsets_ok(off.data(), F), "well formed");
            DotTable tb;
            dot_tile_table(off.data(), F, tb);
            long long nt = 0, nc = 0;
            dot_table_counts(off.data(), F, &nt, &nc);
            CHECK((long long)tb.tiles.size() == nt && tb.cols() == nc && (int)tb.col.size() == F + 1, "counts");
            size_t k = 0;
            for (int f = 0; f < F; ++f) {
                CHECK(tb.col[f] % DOT_TPB == 0 && tb.col[f + 1] - tb.col[f] == dot_cols(ln[f]), "query %d begins a block", f);
                int64_t at = off[f];
                for (int64_t j = 0; j < dot_tiles(ln[f]); ++j, ++k) {
                    const DotTile &t = tb.tiles[k];
                    CHECK(t.e0 == at && t.col == tb.col[f] + j && t.cnt >= 1 && t.cnt <= DOT_WG_SLOTS, "query %d tile %lld", f, (long long)j);
                    CHECK(t.cnt == DOT_WG_SLOTS || j == dot_tiles(ln[f]) - 1, "only the last tile of a query is short");
                    at += t.cnt;
                }
                CHECK(at == off[f + 1], "query %d covered", f);
            }
            CHECK(k == tb.tiles.size(), "no tile beyond the queries");
            // the device input laid out and written whole
            for (bool host_src : {false, true}) {
                const DotSparseWork w = dot_sparse_work(nt, F, off[F], host_src);
                std::vector<unsigned char> buf(w.bytes);
                CHECK(w.off_col == 24 * (size_t)nt && w.off_ids == w.off_col + 8 * ((size_t)F + 1) && w.off_ids % 8 == 0 && w.off_w % 8 == 0, "aligned sections");
                if (nt) std::memcpy(buf.data(), tb.tiles.data(), 24 * (size_t)nt);
                std::memcpy(buf.data() + w.off_col, tb.col.data(), 8 * ((size_t)F + 1));
                if (host_src) {
                    std::memset(buf.data() + w.off_ids, 1, 4 * (size_t)off[F]);
                    std::memset(buf.data() + w.off_w, 2, 8 * (size_t)off[F]);
                    CHECK(w.off_w >= w.off_ids + 4 * (size_t)off[F] && w.bytes == w.off_w + 8 * (size_t)off[F], "ids and w inside");
                } else {
                    CHECK(w.bytes == std::max<size_t>(w.off_ids, 8), "no copy of a device source");
                }
            }
        }
        // counts alone, beyond 2^31 entries
        const int64_t big[] = {0, ((int64_t)1 << 33) + 1, ((int64_t)1 << 33) + 2};
        long long nt = 0, nc = 0;
        dot_table_counts(big, 2, &nt, &nc);
        CHECK(nt == ((long long)1 << 22) + 2 && nc == (((long long)1 << 17) + 1) * 32 + 32, "counts past 2^31 entries");
    }

    // argument and offset checks
    {
        int x = 0;
        const void *P = &x;
        const int64_t good[] = {0, 0, 3, 3, 10}, neg[] = {0, 2, 1, 3, 4}, first[] = {1, 2, 3, 4, 5}, below[] = {0, -1, 3, 4, 5};
        ++cases;
        CHECK(dot_offsets_ok(good, 4) && !dot_offsets_ok(neg, 4) && !dot_offsets_ok(first, 4) && !dot_offsets_ok(below, 4) && !dot_offsets_ok(nullptr, 4), "offsets");
        CHECK(dot_dense_args_ok(0, P, 0, 0, 1, 0, P) && dot_dense_args_ok(1, P, 1, 1, 4096, 1, P), "good dense calls");
        CHECK(!dot_dense_args_ok(2, P, 0, 0, 1, 0, P) && !dot_dense_args_ok(-1, P, 0, 0, 1, 0, P) && !dot_dense_args_ok(0, nullptr, 0, 0, 1, 0, P) &&
                  !dot_dense_args_ok(0, P, 2, 0, 1, 0, P) && !dot_dense_args_ok(0, P, -1, 0, 1, 0, P) && !dot_dense_args_ok(0, P, 0, 2, 1, 0, P) &&
                  !dot_dense_args_ok(0, P, 0, -1, 1, 0, P) && !dot_dense_args_ok(0, P, 0, 0, 0, 0, P) && !dot_dense_args_ok(0, P, 0, 0, 4097, 0, P) &&
                  !dot_dense_args_ok(0, P, 0, 0, -5, 0, P) && !dot_dense_args_ok(0, P, 0, 0, 1, 2, P) && !dot_dense_args_ok(0, P, 0, 0, 1, -1, P) &&
                  !dot_dense_args_ok(0, P, 0, 0, 1, 0, nullptr),
              "bad dense calls");
        CHECK(dot_sparse_args_ok(0, good, P, P, 0, 4, 0, P) && dot_sparse_args_ok(1, good, P, P, 1, 4, 1, P), "good sparse calls");
        CHECK(!dot_sparse_args_ok(2, good, P, P, 0, 4, 0, P) && !dot_sparse_args_ok(0, neg, P, P, 0, 4, 0, P) && !dot_sparse_args_ok(0, nullptr, P, P, 0, 4, 0, P) &&
                  !dot_sparse_args_ok(0, good, nullptr, P, 0, 4, 0, P) && !dot_sparse_args_ok(0, good, P, nullptr, 0, 4, 0, P) &&
                  !dot_sparse_args_ok(0, good, P, P, 2, 4, 0, P) && !dot_sparse_args_ok(0, good, P, P, -1, 4, 0, P) && !dot_sparse_args_ok(0, good, P, P, 0, 0, 0, P) &&
                  !dot_sparse_args_ok(0, good, P, P, 0, 4097, 0, P) && !dot_sparse_args_ok(0, good, P, P, 0, 4, 2, P) && !dot_sparse_args_ok(0, good, P, P, 0, 4, 0, nullptr),
              "bad sparse calls");
        const int32_t ids[] = {0, 9, 4, 9}, lo[] = {0, -1, 3}, hi[] = {0, 10, 3};
        CHECK(ids_in_range(ids, 4, 10) && !ids_in_range(lo, 3, 10) && !ids_in_range(hi, 3, 10) && ids_in_range(hi, 0, 10), "ids");
    }

    // the fold
    {
        std::mt19937_64 rng(12345);
        std::normal_distribution<double> nd(0.0, 1.0);
        for (int64_t m : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)2047, (int64_t)2049, (int64_t)65535, (int64_t)65536,
                          (int64_t)65537, (int64_t)3 * 65536 + 700}) {
            std::vector<double> t((size_t)m + 1);
            for (auto &v : t) v = nd(rng) * std::exp(8.0 * nd(rng));
            ++cases;
            const double want = fold_plain(t.data(), m), got = dot_fold_ref(t.data(), m);
            CHECK(bits(got) == bits(want), "m %lld: %.17g vs %.17g", (long long)m, got, want);
            for (int G : {1, 2, 4, 16, 32, 64, 128, 256}) {
                const double dev = fold_pieces(t.data(), m, G);
                CHECK(bits(dev) == bits(want), "the pieces, m %lld G %d: %.17g vs %.17g", (long long)m, G, dev, want);
            }
            if (m > 1000) { // the order is pinned: a running sum differs
                double run = 0.0;
                for (int64_t j = 0; j < m; ++j) run = add(run, t[(size_t)j]);
                CHECK(bits(run) != bits(want), "m %lld: a running sum gives the same bits", (long long)m);
            }
        }
        // the crafted cancellation: the tree pairs (1e16 + 1) and (-1e16 + 1), each of which loses its 1
        for (int64_t at : {(int64_t)0, (int64_t)254, (int64_t)255, (int64_t)2046, (int64_t)65534, (int64_t)65535}) {
            ++cases;
            std::vector<double> t((size_t)at + 4, 0.0);
            t[(size_t)at] = 1e16, t[(size_t)at + 1] = 1.0, t[(size_t)at + 2] = -1e16, t[(size_t)at + 3] = 1.0;
            const double got = dot_fold_ref(t.data(), at + 4);
            // aligned to a pair: (1e16 + 1) + (-1e16 + 1) = 0, both ones lost
            const double want = fold_plain(t.data(), at + 4);
            CHECK(bits(got) == bits(want), "at %lld", (long long)at);
            if (at % 2 == 0) CHECK(got == 0.0, "at %lld: %.17g", (long long)at, got);
            for (int G : {1, 8, 32, 128, 256}) CHECK(bits(fold_pieces(t.data(), at + 4, G)) == bits(want), "the pieces, at %lld G %d", (long long)at, G);
        }
        // signed zeros: the padding is +0.0 and is added
        const double nz[] = {-0.0, -0.0};
        CHECK(bits(dot_fold_ref(nz, 1)) == bits(0.0) && bits(dot_fold_ref(nz, 2)) == bits(0.0), "-0.0 + padding is +0.0");
        CHECK(bits(dot_fold_ref(nz, 0)) == bits(0.0), "a query without slots is +0.0");
    }
    std::printf("dot_plan_test: %ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
