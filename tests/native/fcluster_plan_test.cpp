// fcluster_plan_test.cpp -- dynamicppr_amd/csrc/dppr_fcluster_plan.hpp on the CPU: the argument check at every limit, the debug
// hook's values, the columns' offsets with max_len and the capacity rule, the block's sections, the tiles of the scan and their
// carries against a plain running sum, the merge of the candidates for the best prefix (ties, none, order of the merge), the bound on
// the piece list against random row lengths, and the host restatement fc_host: on a hand-worked graph here, and on the cases of a
// file (argv[1], written by tests/test_fcluster_plan.py) whose results are printed for the comparison with tests/fcluster_ref.py.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_fcluster_plan.hpp"

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

static const double INF = std::numeric_limits<double>::infinity();

static bool args(int32_t order, double min_score, int64_t max_len, int32_t min_size, int64_t cap, int dest, bool best, bool offsets, int arrays) {
    dppr_fcluster_t b;
    int64_t o;
    int x;
    return fc_args_ok(order, min_score, max_len, 100, min_size, cap, dest, best ? &b : nullptr, offsets ? &o : nullptr, (arrays & 1) ? &x : nullptr,
                      (arrays & 2) ? &x : nullptr, (arrays & 4) ? &x : nullptr, (arrays & 8) ? &x : nullptr, (arrays & 16) ? &x : nullptr);
}

static void arguments() {
    CHECK(args(0, 0.0, 0, 1, 0, DPPR_DEST_HOST, true, true, 0) && args(1, 1e-9, 100, 7, 5, DPPR_DEST_DEVICE, true, true, 16), "the limits themselves");
    CHECK(!args(2, 0.0, 0, 1, 0, 0, true, true, 0) && !args(-1, 0.0, 0, 1, 0, 0, true, true, 0), "order");
    CHECK(!args(0, -1e-300, 0, 1, 0, 0, true, true, 0) && !args(0, std::nan(""), 0, 1, 0, 0, true, true, 0) && args(0, -0.0, 0, 1, 0, 0, true, true, 0),
          "min_score");
    CHECK(!args(0, 0.0, -1, 1, 0, 0, true, true, 0) && !args(0, 0.0, 101, 1, 0, 0, true, true, 0) && args(0, 0.0, 100, 1, 0, 0, true, true, 0), "max_len");
    CHECK(!args(0, 0.0, 0, 0, 0, 0, true, true, 0) && !args(0, 0.0, 0, -2, 0, 0, true, true, 0) && args(0, 0.0, 0, 1000, 0, 0, true, true, 0), "min_size");
    CHECK(!args(0, 0.0, 0, 1, -1, 0, true, true, 1) && !args(0, 0.0, 0, 1, 1, 0, true, true, 0), "cap");
    for (int a = 1; a < 32; a <<= 1) CHECK(args(0, 0.0, 0, 1, 1, 0, true, true, a), "cap > 0 with one array: %d", a);
    CHECK(!args(0, 0.0, 0, 1, 0, 2, true, true, 0) && !args(0, 0.0, 0, 1, 0, -1, true, true, 0), "dest");
    CHECK(!args(0, 0.0, 0, 1, 0, 0, false, true, 0) && !args(0, 0.0, 0, 1, 0, 0, true, false, 0), "best / offsets");
    CHECK(fc_hook_ok(0) && fc_hook_ok(64) && fc_hook_ok(4096) && fc_hook_ok(1024) && !fc_hook_ok(32) && !fc_hook_ok(8192) && !fc_hook_ok(96) && !fc_hook_ok(-64),
          "the hook's values");
    CHECK(fc_scan_tile(0) == FC_SCAN_TILE && fc_scan_tile(64) == 64 && fc_piece(0) == FC_PIECE && fc_piece(128) == 128, "0: the plan decides");
    CHECK(fc_cap_clamped(5, 10, 3) == 5 && fc_cap_clamped(31, 10, 3) == 30 && fc_cap_clamped(INT64_MAX, 1 << 30, 16) == (int64_t)16 << 30, "cap clamp");
}

static void scores() {
    CHECK(fc_score(DPPR_FCLUSTER_BY_P, 0.3, 7) == 0.3 && fc_score(DPPR_FCLUSTER_BY_P_OVER_DEG, 0.3, 7) == 0.3 / 8.0, "one division");
    CHECK(fc_score(DPPR_FCLUSTER_BY_P_OVER_DEG, 1.0, 0) == 1.0, "degree 0");
    CHECK(!fc_qualifies(-1.0, 0.0, true) && !fc_qualifies(0.0, 0.0, true) && !fc_qualifies(-0.0, 0.0, true) && !fc_qualifies(std::nan(""), 0.0, true),
          "negative, zero, NaN");
    CHECK(fc_qualifies(INF, 0.0, true) && fc_qualifies(5e-324, 0.0, true) && !fc_qualifies(1e-6, 1e-6, true) && !fc_qualifies(1.0, 0.0, false), "strict, named");
}

static void columns() {
    const long long q[4] = {0, 10, 10, 75};
    FcCols c = fc_cols(q, 3, 0, 64);
    CHECK(c.m == 3 && c.off[0] == 0 && c.off[1] == 10 && c.off[2] == 10 && c.off[3] == 75 && c.off[16] == 75, "max_len 0: every qualifying vertex");
    CHECK(c.tile0[1] == 1 && c.tile0[2] == 1 && c.tile0[3] == 3 && c.tile0[16] == 3, "tiles: %lld %lld %lld", c.tile0[1], c.tile0[2], c.tile0[3]);
    CHECK(c.qoff[1] == 10 && c.qoff[3] == 75 && c.qoff[16] == 75, "the sort's ranges");
    c = fc_cols(q, 3, 37, 64);
    CHECK(c.off[1] == 10 && c.off[2] == 10 && c.off[3] == 47 && c.qoff[2] == 10 && c.qoff[3] == 75 && c.tile0[3] == 2, "max_len 37");
    c = fc_cols(q, 3, 64, 64);
    CHECK(c.off[3] == 74 && c.tile0[3] - c.tile0[2] == 1, "a column of exactly one tile");
    CHECK(fc_len(5, 0) == 5 && fc_len(5, 5) == 5 && fc_len(5, 4) == 4 && fc_len(0, 3) == 0, "fc_len");
    CHECK(fc_fits(0, 0) && fc_fits(7, 7) && !fc_fits(8, 7), "the capacity rule");
    for (int64_t T : {0, 1, 2, 3, 1000}) {
        const FcLayout l = fc_layout(T);
        CHECK(l.off_ids == 0 && l.off_score >= 4 * (size_t)T && l.off_score % 8 == 0 && l.off_cut_out == l.off_score + 8 * (size_t)T &&
                  l.off_cut_in == l.off_cut_out + 8 * (size_t)T && l.off_vol == l.off_cut_in + 8 * (size_t)T && l.total_bytes == l.off_vol + 8 * (size_t)T,
              "sections of %lld entries", (long long)T);
    }
    CHECK(FC_HEAD_OFF_CTL == 144 && FC_HEAD_OFF_BEST == 160 && FC_HEAD_BYTES == 160 + 640, "the head");
}

static void pieces() {
    CHECK(fc_pieces(65, 64) == 2 && fc_pieces(128, 64) == 2 && fc_pieces(129, 64) == 3, "pieces");
    uint64_t x = 88172645463325252ull;
    for (int round = 0; round < 200; ++round)
        for (int piece : {64, 2048, 4096}) {
            long long Ed = 0, n = 0;
            const int rows = 1 + round % 37;
            for (int r = 0; r < rows; ++r) {
                x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                const long long len = (long long)(x % (unsigned)(round % 3 == 0 ? 3 * piece : 40 * piece));
                Ed += len;
                if (len > piece) n += fc_pieces(len, piece);
            }
            for (int m : {1, 3, 16}) CHECK((size_t)(2 * m * n) <= fc_list_cap(m, Ed, piece), "round %d: %lld pieces, Ed %lld", round, n, Ed);
        }
}

static void merge() {
    const FcBest none = fc_none(), a{0.25, 3, 2, 8}, b{0.25, 1, 2, 8}, c{0.125, 9, 1, 8};
    CHECK(fc_merge(none, none).pos < 0 && fc_merge(none, a).pos == 3 && fc_merge(a, none).pos == 3, "none");
    CHECK(fc_merge(a, b).pos == 1 && fc_merge(b, a).pos == 1, "equal phi: the smaller position, whichever comes first");
    CHECK(fc_merge(a, c).pos == 9 && fc_merge(c, a).pos == 9, "smaller phi wins");
    CHECK(fc_candidate(0, 3, 3, 20, 1).phi == 1.0 && fc_candidate(0, 3, 3, 20, 2).pos < 0 && fc_candidate(5, 0, 20, 20, 1).pos < 0 &&
              fc_candidate(5, 0, 0, 20, 1).pos < 0,
          "eligibility");
    CHECK(fc_candidate(2, 3, 489, 1492, 1).phi == 3.0 / 489.0 && fc_candidate(2, 3, 1003, 1492, 1).phi == 3.0 / 489.0, "one division, den = min(vol, Ed - vol)");
    const dppr_fcluster_t r0 = fc_record(7, none), r1 = fc_record(7, a);
    CHECK(r0.count == 7 && r0.best_size == 0 && r0.best_cut == 0 && r0.best_vol == 0 && r0.best_phi == INF, "no eligible prefix");
    CHECK(r1.best_size == 4 && r1.best_cut == 2 && r1.best_vol == 8 && r1.best_phi == 0.25, "a record");
}

// two triangles {0,1,2} and {3,4,5} joined by 2 -> 3 and 3 -> 2, both directions stored; vertex 6 has a self loop only, 7 no edge
static FcCsr two_triangles() {
    FcCsr g;
    g.V = 8;
    const std::vector<std::vector<int>> rows = {{1, 2}, {0, 2}, {0, 1, 3}, {2, 4, 5}, {3, 5}, {3, 4}, {6}, {}};
    g.ptr.push_back(0);
    for (const auto &r : rows) {
        for (int w : r) g.col.push_back(w);
        g.ptr.push_back((int64_t)g.col.size());
    }
    return g;
}

static void restatement() {
    const FcCsr g = two_triangles();
    const double nan = std::nan("");
    // by p: 0 (0.5), 1 and 2 tie at 0.25 (id order), 3 (0.1), 6 (0.05); 4 negative, 5 NaN, 7 unnamed with the largest p
    const std::vector<double> p = {0.5, 0.25, 0.25, 0.1, -0.3, nan, 0.05, 9.0};
    for (int tile : {1, 2, 3, 64}) {
        const FcResult r = fc_host(g, p.data(), DPPR_FCLUSTER_BY_P, 0.0, 0, 1, tile);
        CHECK(r.ids == (std::vector<int32_t>{0, 1, 2, 3, 6}), "order, tile %d", tile);
        CHECK(r.vol == (std::vector<int64_t>{2, 4, 7, 10, 11}), "vol, tile %d", tile);
        CHECK(r.cut_out == (std::vector<int64_t>{2, 2, 1, 2, 2}), "cut_out, tile %d: %lld %lld %lld %lld %lld", tile, (long long)r.cut_out[0],
              (long long)r.cut_out[1], (long long)r.cut_out[2], (long long)r.cut_out[3], (long long)r.cut_out[4]);
        CHECK(r.cut_in == r.cut_out, "both directions stored, tile %d", tile);
        // Ed = 15: den 2 4 7 5 4; phi 1, .5, 1/7, .4, .5
        CHECK(r.best.count == 5 && r.best.best_size == 3 && r.best.best_cut == 1 && r.best.best_vol == 7 && r.best.best_phi == 1.0 / 7.0, "best, tile %d", tile);
    }
    FcResult r = fc_host(g, p.data(), DPPR_FCLUSTER_BY_P, 0.0, 2, 1, 64);
    CHECK(r.ids == (std::vector<int32_t>{0, 1}) && r.cut_out == (std::vector<int64_t>{2, 2}) && r.best.best_size == 2 && r.best.count == 2, "max_len 2: the head");
    r = fc_host(g, p.data(), DPPR_FCLUSTER_BY_P, 0.1, 0, 4, 64);
    CHECK(r.ids == (std::vector<int32_t>{0, 1, 2}) && r.best.best_size == 0 && r.best.best_phi == INF && r.best.count == 3, "min_score strict, min_size above L");
    // by p / (deg + 1): 0: .5/3, 1: .25/3, 2: .25/4, 3: .1/4, 6: .05/2 = .025 = 3's score: 3 before 6 by id
    r = fc_host(g, p.data(), DPPR_FCLUSTER_BY_P_OVER_DEG, 0.0, 0, 1, 2);
    CHECK(r.ids == (std::vector<int32_t>{0, 1, 2, 3, 6}) && r.score[3] == 0.1 / 4.0 && r.score[4] == 0.05 / 2.0 && r.score[0] == 0.5 / 3.0, "by degree");
    std::vector<double> inf_p = p;
    inf_p[6] = INF;
    r = fc_host(g, inf_p.data(), DPPR_FCLUSTER_BY_P, 0.0, 0, 1, 64);
    CHECK(r.ids[0] == 6 && r.cut_out[0] == 0 && r.vol[0] == 1 && r.best.best_size == 1 && r.best.best_phi == 0.0, "+inf orders first; a self loop never crosses");
    const std::vector<double> zero(8, 0.0);
    r = fc_host(g, zero.data(), DPPR_FCLUSTER_BY_P, 0.0, 0, 1, 64);
    CHECK(r.ids.empty() && r.best.count == 0 && r.best.best_size == 0 && r.best.best_phi == INF, "an empty order");
}

// the scan's tiles and carries against one running sum, every tile size
static void tiles() {
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (int L : {0, 1, 63, 64, 65, 200}) {
        std::vector<long long> d((size_t)L), run((size_t)L);
        long long s = 0;
        for (int j = 0; j < L; ++j) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            d[(size_t)j] = (long long)(x % 11) - 5;
            run[(size_t)j] = s += d[(size_t)j];
        }
        for (int tile : {1, 7, 64, 256}) {
            const long long q[2] = {0, L};
            const FcCols c = fc_cols(q, 1, 0, tile);
            const long long nt = c.tile0[1];
            CHECK(nt == (L + tile - 1) / tile, "tiles of %d positions by %d", L, tile);
            long long carry = 0;
            for (long long t = 0; t < nt; ++t) {
                long long v = carry;
                for (long long j = t * tile; j < L && j < (t + 1) * tile; ++j) {
                    v += d[(size_t)j];
                    CHECK(v == run[(size_t)j], "position %lld, tile %d", j, tile);
                }
                carry = v;
            }
        }
    }
}

static uint64_t hex(const char *s) { return std::strtoull(s, nullptr, 16); }

// the case file: "V Ed" | ptr [V + 1] | col [Ed] | n_cases | per case: "order min_score(hex) max_len min_size scan_tile" then p (hex) [V]
static int run_file(const char *path) {
    FILE *f = std::fopen(path, "r");
    if (!f) return 1;
    FcCsr g;
    long long V, Ed, n;
    char w[64];
    if (std::fscanf(f, "%lld %lld", &V, &Ed) != 2) return 1;
    g.V = V;
    g.ptr.resize((size_t)V + 1);
    g.col.resize((size_t)Ed);
    for (auto &v : g.ptr) { long long t; if (std::fscanf(f, "%lld", &t) != 1) return 1; v = t; }
    for (auto &v : g.col) { int t; if (std::fscanf(f, "%d", &t) != 1) return 1; v = t; }
    if (std::fscanf(f, "%lld", &n) != 1) return 1;
    for (long long i = 0; i < n; ++i) {
        int order, min_size, tile;
        long long max_len;
        if (std::fscanf(f, "%d %63s %lld %d %d", &order, w, &max_len, &min_size, &tile) != 5) return 1;
        const uint64_t ms = hex(w);
        double min_score;
        std::memcpy(&min_score, &ms, 8);
        std::vector<double> p((size_t)V);
        for (auto &v : p) {
            if (std::fscanf(f, "%63s", w) != 1) return 1;
            const uint64_t b = hex(w);
            std::memcpy(&v, &b, 8);
        }
        const FcResult r = fc_host(g, p.data(), order, min_score, max_len, min_size, tile);
        uint64_t phi;
        std::memcpy(&phi, &r.best.best_phi, 8);
        std::printf("res %lld %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %016" PRIx64, i, r.best.count, r.best.best_size, r.best.best_cut, r.best.best_vol, phi);
        for (size_t j = 0; j < r.ids.size(); ++j) {
            uint64_t s;
            std::memcpy(&s, &r.score[j], 8);
            std::printf(" %d %016" PRIx64 " %" PRId64 " %" PRId64 " %" PRId64, r.ids[j], s, r.cut_out[j], r.cut_in[j], r.vol[j]);
        }
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    arguments();
    scores();
    columns();
    pieces();
    merge();
    restatement();
    tiles();
    if (argc > 1 && run_file(argv[1])) {
        ++failures;
        std::printf("FAIL the case file\n");
    }
    std::printf("fcluster_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
