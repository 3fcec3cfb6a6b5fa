// fpush_plan_test.cpp -- dynamicppr_amd/csrc/dppr_fpush_plan.hpp on the CPU: every rejection of a call's arguments and of the start
// sets' CSR at its limit, which parts a call asks for and when a part is complete, the hook's values, the chunk schedule against its
// plain statement, the sizes of the bitmap and the lists, the insertion of a host-answered seed into a top-k list, and the host
// round on a hand-made graph: worked by hand, and printed (`round` lines) for tests/test_fpush_plan.py to hold against
// tests/fpush_ref.py bit for bit. Every array is exactly as long as the code may touch (the sanitizers watch the bounds).
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_fpush_plan.hpp"

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
    dppr_forward_push_out_t out{};
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(fp_args_ok(1, 1e-300, 1, &out) && fp_args_ok(16, 1e-6, 256, &out) && fp_args_ok(3, std::numeric_limits<double>::max(), 8, &out),
          "the limits are inside");
    CHECK(!fp_args_ok(0, 1e-6, 8, &out) && !fp_args_ok(17, 1e-6, 8, &out) && !fp_args_ok(-1, 1e-6, 8, &out), "m outside 1 .. 16");
    CHECK(!fp_args_ok(1, 0.0, 8, &out) && !fp_args_ok(1, -0.0, 8, &out) && !fp_args_ok(1, -1e-6, 8, &out) && !fp_args_ok(1, std::nan(""), 8, &out) &&
              !fp_args_ok(1, inf, 8, &out) && !fp_args_ok(1, -inf, 8, &out),
          "an eps that is not finite or not > 0");
    CHECK(!fp_args_ok(1, 1e-6, 0, &out) && !fp_args_ok(1, 1e-6, 257, &out) && !fp_args_ok(1, 1e-6, -3, &out), "max_rounds outside 1 .. 256");
    CHECK(!fp_args_ok(1, 1e-6, 8, nullptr), "a NULL out");
    CHECK(fp_hook_ok(0, 0, 0) && fp_hook_ok(64, 1, 1) && fp_hook_ok(4096, 8, 256) && fp_hook_ok(512, 2, 3), "the hook's values");
    CHECK(!fp_hook_ok(32, 0, 0) && !fp_hook_ok(96, 0, 0) && !fp_hook_ok(8192, 0, 0) && !fp_hook_ok(0, 3, 0) && !fp_hook_ok(0, 16, 0) &&
              !fp_hook_ok(0, 0, -1) && !fp_hook_ok(0, 0, 257),
          "the hook's rejections");
}

static void csr() {
    const int64_t V = 10;
    { // exactly as long as the offsets say
        const std::vector<int64_t> off{0, 1, 3};
        const std::vector<int32_t> ids{4, 9, 0};
        const std::vector<double> w{1.0, 0.25, 1e300};
        CHECK(fp_csr_check(off.data(), ids.data(), w.data(), 2, V) == TG_OK, "a good CSR; an id in two columns is fine");
        CHECK(fp_csr_check(nullptr, ids.data(), w.data(), 2, V) == TG_NULL && fp_csr_check(off.data(), nullptr, w.data(), 2, V) == TG_NULL &&
                  fp_csr_check(off.data(), ids.data(), nullptr, 2, V) == TG_NULL,
              "a NULL array");
        CHECK(fp_csr_check(off.data(), ids.data(), w.data(), 0, V) == TG_BAD_N && fp_csr_check(off.data(), ids.data(), w.data(), 17, V) == TG_BAD_N,
              "m is checked before anything is read");
        CHECK(fp_csr_check(off.data(), ids.data(), w.data(), 2, 9) == TG_BAD_ID, "an id at V");
    }
    const std::vector<int32_t> ids{1, 2, 3};
    const std::vector<double> w{1.0, 2.0, 3.0};
    const auto with_off = [&](std::vector<int64_t> off) { return fp_csr_check(off.data(), ids.data(), w.data(), 2, V); };
    CHECK(with_off({1, 2, 3}) == TG_BAD_OFFSETS && with_off({0, 2, 1}) == TG_BAD_OFFSETS && with_off({0, -1, 3}) == TG_BAD_OFFSETS,
          "offsets that do not start at 0 or decrease");
    CHECK(with_off({0, 0, 3}) == TG_BAD_SIZE && with_off({0, 3, 3}) == TG_BAD_SIZE, "an empty column");
    const auto with = [&](std::vector<int32_t> i, std::vector<double> x) {
        const std::vector<int64_t> off{0, 1, 3};
        return fp_csr_check(off.data(), i.data(), x.data(), 2, V);
    };
    CHECK(with({1, 2, -1}, {1, 1, 1}) == TG_BAD_ID && with({1, 5, 5}, {1, 1, 1}) == TG_DUP_ID && with({5, 5, 6}, {1, 1, 1}) == TG_OK,
          "an id out of range, an id twice in a column, the same id in two columns");
    CHECK(with({1, 2, 3}, {1, 0.0, 1}) == TG_BAD_WEIGHT && with({1, 2, 3}, {-1, 1, 1}) == TG_BAD_WEIGHT &&
              with({1, 2, 3}, {1, 1, std::nan("")}) == TG_BAD_WEIGHT && with({1, 2, 3}, {std::numeric_limits<double>::infinity(), 1, 1}) == TG_BAD_WEIGHT,
          "a weight that is not finite or not > 0");
    { // FP_SET_MAX seeds are a column, one more is not (the size is refused before an id is read)
        std::vector<int32_t> many(FP_SET_MAX);
        for (int i = 0; i < FP_SET_MAX; ++i) many[(size_t)i] = i;
        const std::vector<double> ones(FP_SET_MAX, 1.0);
        const std::vector<int64_t> ok{0, FP_SET_MAX}, over{0, FP_SET_MAX + 1};
        CHECK(fp_csr_check(ok.data(), many.data(), ones.data(), 1, FP_SET_MAX) == TG_OK, "FP_SET_MAX seeds");
        CHECK(fp_csr_check(over.data(), many.data(), ones.data(), 1, FP_SET_MAX) == TG_BAD_SIZE, "FP_SET_MAX + 1 seeds");
    }
}

static void parts() {
    dppr_forward_push_out_t o{};
    int32_t i = 0;
    int64_t l = 0;
    double d = 0;
    CHECK(fp_which(nullptr) == 0 && fp_which(&o) == 0 && fp_parts_ok(&o), "nothing asked: nothing to complete");
    o.left = &l;
    CHECK(fp_which(&o) == FP_META && fp_parts_ok(&o), "left alone");
    o.left = nullptr, o.work = &l;
    CHECK(fp_which(&o) == FP_WORK && fp_parts_ok(&o), "work alone");
    o.topk_p = &d;
    CHECK(fp_which(&o) == (FP_WORK | FP_TOPK) && !fp_parts_ok(&o), "a top-k part with pointers missing");
    o.topk_ids = &i, o.topk_counts = &i, o.k = 0;
    CHECK(!fp_parts_ok(&o), "k = 0");
    o.k = DPPR_TOPK_MAX + 1;
    CHECK(!fp_parts_ok(&o), "k beyond DPPR_TOPK_MAX");
    o.k = 1, o.min_p = -1e-9;
    CHECK(!fp_parts_ok(&o), "a negative min_p");
    o.min_p = std::nan("");
    CHECK(!fp_parts_ok(&o), "a NaN min_p");
    o.min_p = 0.0;
    CHECK(fp_parts_ok(&o), "a complete top-k part");
    o.at_r = &d;
    CHECK((fp_which(&o) & FP_AT) && !fp_parts_ok(&o), "at_r without ids");
    o.at_ids = &i, o.n_at = 0;
    CHECK(!fp_parts_ok(&o), "n_at = 0");
    o.n_at = DPPR_FORWARD_AT_MAX + 1;
    CHECK(!fp_parts_ok(&o), "n_at beyond the limit");
    o.n_at = DPPR_FORWARD_AT_MAX;
    CHECK(fp_parts_ok(&o), "r alone at the ids");
    o.at_r = nullptr;
    CHECK((fp_which(&o) & FP_AT) && !fp_parts_ok(&o), "ids with neither p nor r");
    o.at_p = &d;
    CHECK(fp_parts_ok(&o), "p alone at the ids");
    o.dense_r_dev = &d;
    CHECK((fp_which(&o) & FP_DENSE) && fp_parts_ok(&o), "r alone as a dense copy");
    o.dense_dtype = 2;
    CHECK(!fp_parts_ok(&o), "a dtype that does not exist");
    o.dense_dtype = DPPR_F32, o.dense_layout = 2;
    CHECK(!fp_parts_ok(&o), "a layout that does not exist");
}

static void schedule() {
    for (int chunk = 1; chunk <= FP_MAX_ROUNDS; ++chunk)
        for (int max_rounds = 1; max_rounds <= FP_MAX_ROUNDS; ++max_rounds) {
            int k = 0, reads = 0;
            while (k < max_rounds) {
                const int end = fp_chunk_end(k, max_rounds, chunk);
                CHECK(end > k && end <= max_rounds && end - k <= chunk && (end == max_rounds || end - k == chunk), "chunk %d max %d k %d", chunk, max_rounds, k);
                k = end;
                ++reads;
            }
            CHECK(k == max_rounds && reads == fp_chunks(max_rounds, chunk), "chunk %d max %d: %d read-backs", chunk, max_rounds, reads);
        }
    CHECK(fp_chunk(0) == FP_CHUNK && fp_chunk(1) == 1 && fp_chunk(256) == 256, "0 leaves the chunk to the plan");
}

static void sizes() {
    CHECK(fp_bitmap_words(0) == 1 && fp_bitmap_words(1) == 1 && fp_bitmap_words(32) == 1 && fp_bitmap_words(33) == 2 &&
              fp_bitmap_words(((int64_t)1 << 31) - 1) == ((size_t)1 << 26),
          "a bit per row");
    CHECK(fp_list_cap(0) == 1 && fp_list_cap(1000) == 1000, "a row enters a list once");
    // the pieces of the out-rows of ANY frontier fit the list: sum of ceil(d / P) <= rows + edges / P
    for (long long d : {0ll, 1ll, 127ll, 128ll, 129ll, 1000000ll})
        CHECK(fp_mark_pieces(d) == (d + FP_MARK_PIECE - 1) / FP_MARK_PIECE && fp_mark_pieces(d) * FP_MARK_PIECE >= d &&
                  (size_t)(3 * fp_mark_pieces(d)) <= fp_mark_cap(3, 3 * d),
              "out-degree %lld", d);
    CHECK(fp_grid(0, 256) == 1 && fp_grid(257, 256) == 2 && fp_grid(1ll << 40, 256) == FP_GRID_MAX, "grids are bounded");
    CHECK(sizeof(FpSeed) == 24 && offsetof(FpHead, fw) == 0 && offsetof(FpHead, last_act) % 4 == 0 && offsetof(FpHead, pushes) % 8 == 0, "the head's layout");
}

static void topk_insert() {
    std::vector<int32_t> ids{7, 3, -1, -1};
    std::vector<double> ps{0.5, 0.2, 0.0, 0.0};
    int n = fp_topk_insert(ids.data(), ps.data(), 2, 4, 0.0, 9, 0.3);
    CHECK(n == 3 && ids[0] == 7 && ids[1] == 9 && ids[2] == 3 && ps[1] == 0.3 && ps[2] == 0.2, "between two entries");
    n = fp_topk_insert(ids.data(), ps.data(), n, 4, 0.0, 1, 0.3);
    CHECK(n == 4 && ids[1] == 1 && ids[2] == 9 && ids[3] == 3, "a tie goes by id ascending");
    n = fp_topk_insert(ids.data(), ps.data(), n, 4, 0.0, 5, 0.25);
    CHECK(n == 4 && ids[3] == 5 && ps[3] == 0.25, "a full list drops its last");
    n = fp_topk_insert(ids.data(), ps.data(), n, 4, 0.0, 6, 0.1);
    CHECK(n == 4 && ids[3] == 5, "below a full list: not taken");
    n = fp_topk_insert(ids.data(), ps.data(), n, 4, 0.9, 8, 0.9);
    CHECK(n == 4 && ids[0] == 7, "p > min_p is strict");
    std::vector<int32_t> one{-1};
    std::vector<double> onep{0.0};
    CHECK(fp_topk_insert(one.data(), onep.data(), 0, 1, 0.0, 4, 0.15) == 1 && one[0] == 4 && onep[0] == 0.15, "into an empty list of one");
    CHECK(fp_rowless_p(1.0) == 0.15 && fp_rowless_p(3.0) == 0.15 * 3.0, "p of a seed without a row");
}

// 0 -> 1, 0 -> 2, 1 -> 2, 2 -> 0, 2 -> 2 (a self loop), 1 -> 2 again (a duplicate), 3 -> 0; 4 has no edge. In-CSR by head.
static const int V = 5;
static const int PTR[V + 1] = {0, 2, 3, 7, 7, 7};
static const int TAIL[7] = {2, 3, 0, 0, 1, 1, 2};
static const int D[V] = {2, 2, 2, 1, 0};

static void round_by_hand() {
    std::vector<double> p(V, 0.0), r(V, 0.0), y(V, 0.0);
    r[0] = 1.0;
    const long long n1 = fp_round_ref(V, PTR, TAIL, D, 0.1, p.data(), r.data(), y.data(), FW_PIECE);
    const double y0 = (0.85 * 1.0) / 3.0;
    CHECK(n1 == 1 && p[0] == 0.15 && r[0] == 0.0 && r[1] == y0 && r[2] == y0 && r[3] == 0.0 && r[4] == 0.0, "round 1: 0 pushes to 1 and 2");
    // round 2: thr = 0.3 for 1 and 2; y0 = 0.2833.. stays below: nothing is pushed and nothing changes
    const std::vector<double> p1 = p, r1 = r;
    const long long n2 = fp_round_ref(V, PTR, TAIL, D, 0.1, p.data(), r.data(), y.data(), FW_PIECE);
    CHECK(n2 == 0 && std::memcmp(p.data(), p1.data(), sizeof(double) * V) == 0 && std::memcmp(r.data(), r1.data(), sizeof(double) * V) == 0,
          "an empty frontier changes no bit");
    // with eps = 0.05 both are pushed; 2 receives from 1 twice (the duplicate) and from itself
    const long long n3 = fp_round_ref(V, PTR, TAIL, D, 0.05, p.data(), r.data(), y.data(), FW_PIECE);
    const double y1 = (0.85 * y0) / 3.0;
    CHECK(n3 == 2 && p[1] == 0.15 * y0 && p[2] == 0.15 * y0 && r[1] == 0.0, "round 3: 1 and 2 are pushed");
    CHECK(r[0] == y1 && r[2] == fw_add(fw_add(0.0, y1), fw_add(y1, y1)), "the fold of (y0, y1, y1, y2) by neighbours: the self loop and the duplicate count");
}

static void round_lines() {
    // the rounds of three columns, bit patterns in hex: tests/test_fpush_plan.py runs tests/fpush_ref.py over the same graph
    const struct { int ids[2]; double w[2]; int n; double eps; } cols[3] = {{{0, 0}, {1.0, 0.0}, 1, 1e-3}, {{3, 1}, {0.7, 2.5}, 2, 1e-2}, {{2, 0}, {1e-4, 0.0}, 1, 1e-3}};
    for (int c = 0; c < 3; ++c) {
        std::vector<double> p(V, 0.0), r(V, 0.0), y(V, 0.0);
        for (int j = 0; j < cols[c].n; ++j) r[(size_t)cols[c].ids[j]] = cols[c].w[j];
        for (int k = 1; k <= 12; ++k) {
            const long long n = fp_round_ref(V, PTR, TAIL, D, cols[c].eps, p.data(), r.data(), y.data(), k % 2 ? FW_PIECE_MIN : FW_PIECE_MAX);
            std::printf("round %d %d %lld", c, k, n);
            for (int u = 0; u < V; ++u) {
                uint64_t a, b;
                std::memcpy(&a, &p[(size_t)u], 8);
                std::memcpy(&b, &r[(size_t)u], 8);
                std::printf(" %016" PRIx64 " %016" PRIx64, a, b);
            }
            std::printf("\n");
        }
    }
}

int main() {
    arguments();
    csr();
    parts();
    schedule();
    sizes();
    topk_insert();
    round_by_hand();
    round_lines();
    std::printf("fpush_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
