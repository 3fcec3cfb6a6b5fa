// ftrack_plan_test.cpp -- dynamicppr_amd/csrc/dppr_ftrack_plan.hpp on the CPU: the limits, the outputs of a call seen as those of a
// forward push, the epochs an update accepts, where the first round's candidates come from, the sizes, the fix-up worked by hand,
// and -- given a case file (tests/test_ftrack_plan.py writes it) -- the host restatement of create, fix-up and signed rounds over
// every epoch of the case, printed (`state` lines) to be held against tests/ftrack_ref.py bit for bit. Every array is exactly as
// long as the code may touch (the sanitizers watch the bounds).
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_ftrack_plan.hpp"

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

static void plan() {
    CHECK(FT_MAX == 16 && ft_handle_ok(0) && ft_handle_ok(15) && !ft_handle_ok(16) && !ft_handle_ok(-1), "handles 0 .. 15");
    CHECK(ft_create_args_ok(1, 1e-300, 1) && ft_create_args_ok(16, 1e-6, 256) && !ft_create_args_ok(0, 1e-6, 8) && !ft_create_args_ok(17, 1e-6, 8) &&
              !ft_create_args_ok(1, 0.0, 8) && !ft_create_args_ok(1, std::nan(""), 8) && !ft_create_args_ok(1, 1e-6, 0) && !ft_create_args_ok(1, 1e-6, 257),
          "create takes what dppr_forward_push takes");
    CHECK(ft_rounds_ok(1) && ft_rounds_ok(256) && !ft_rounds_ok(0) && !ft_rounds_ok(257), "max_rounds in 1 .. 256");
    CHECK(ft_step(4, 4) == FT_STEP_SAME && ft_step(4, 5) == FT_STEP_NEXT && ft_step(4, 6) == FT_STEP_BAD && ft_step(4, 3) == FT_STEP_BAD &&
              ft_step(0, 0) == FT_STEP_SAME && ft_step(0, 1) == FT_STEP_NEXT,
          "the own epoch and the next one, nothing else");
    CHECK(ft_candidates_from_records(FT_STEP_NEXT, true) && !ft_candidates_from_records(FT_STEP_NEXT, false) &&
              !ft_candidates_from_records(FT_STEP_SAME, true) && !ft_candidates_from_records(FT_STEP_SAME, false),
          "the records name the candidates only after a fix-up on a converged track");
    CHECK(ft_state_elems(10, 2) == 40 && ft_state_elems(0, 1) == 2 && ft_sort_words(0) == 6 && ft_sort_words(200) == 1200 && ft_c_elems(200, 16) == 3200 &&
              ft_c_elems(0, 1) == 1,
          "sizes");
    // the parts of a call
    CHECK(ft_which(nullptr) == 0 && ft_parts_ok(nullptr), "no outputs is a call");
    dppr_ftrack_out_t o{};
    CHECK(ft_which(&o) == 0 && ft_parts_ok(&o), "an empty struct asks for nothing");
    int64_t fix[3];
    double rem[2];
    o.fix = fix;
    CHECK(ft_which(&o) == FT_FIX, "fix alone");
    o.rem = rem;
    CHECK(ft_which(&o) == (FT_FIX | FP_META), "fix and meta");
    int32_t ids[4];
    o.topk_ids = ids;
    CHECK((ft_which(&o) & FP_TOPK) && !ft_parts_ok(&o), "half a top k is refused");
    o.topk_ids = nullptr;
    o.at_ids = ids;
    o.n_at = 4;
    CHECK((ft_which(&o) & FP_AT) && !ft_parts_ok(&o), "point reads without a destination are refused");
    o.at_p = rem;
    CHECK(ft_parts_ok(&o), "point reads");
    o.n_at = 0;
    CHECK(!ft_parts_ok(&o), "n_at = 0");
}

// 0 -> 1, 0 -> 2, 1 -> 2 becomes 0 -> 1, 1 -> 2, 1 -> 1, 3 -> 2 by: delete 0 -> 2, insert 1 -> 1, insert 3 -> 2
static void by_hand() {
    double p[4] = {0.3, 0.06, 0.0, 0.0}, r[4] = {0.0, 0.25, 0.5, 0.0};
    const int d1[4] = {1, 2, 0, 1}, tail[3] = {0, 1, 3}, head[3] = {2, 1, 2};
    const unsigned char ins[3] = {0, 1, 1};
    long long fix[3];
    ft_fixup_ref(4, p, r, d1, 3, tail, head, ins, fix);
    CHECK(fix[0] == 3 && fix[1] == 3 && fix[2] == 2, "three records, tails 0 1 3, heads 1 2");
    // tail 0: d0 = 2, g = 0.3 / (0.15 * 3), c = 0.85 g; p = 0.3 * 2 / 3; r = 0 + g. tail 1: d0 = 1, g = 0.06 / 0.3, p = 0.06 * 3 / 2,
    // r = 0.25 - g, then + c[1] as the head of its own loop. tail 3: p = 0: nothing moves. head 2: - c[0], + c[3] = +0
    volatile double a0 = 0.15 * 3.0, g0 = 0.3 / a0, c0 = 0.85 * g0, p0 = (0.3 * 2.0) / 3.0, r0 = 0.0 - (-1.0) * g0;
    volatile double a1 = 0.15 * 2.0, g1 = 0.06 / a1, c1 = 0.85 * g1, p1 = (0.06 * 3.0) / 2.0, r1 = 0.25 - g1;
    volatile double r1b = r1 + c1, r2 = 0.5 - c0, r2b = r2 + 0.0;
    CHECK(p[0] == p0 && r[0] == r0 && p[1] == p1 && r[1] == r1b && r[2] == r2b && p[2] == 0.0 && p[3] == 0.0 && r[3] == 0.0, "worked by hand");
    CHECK(!std::signbit(r[3]) && !std::signbit(p[3]), "a vertex new in the batch keeps +0.0");
    // d1 == d0: the tail keeps its bits
    double p2[2] = {0.123, 0.0}, r2v[2] = {0.017, 0.0};
    const int dd[2] = {3, 0}, t2[2] = {0, 0}, h2[2] = {1, 1};
    const unsigned char i2[2] = {1, 0};
    ft_fixup_ref(2, p2, r2v, dd, 2, t2, h2, i2, nullptr);
    volatile double a = 0.15 * 4.0, g = 0.123 / a, c = 0.85 * g, x = 0.0 + c, y = x - c;
    CHECK(p2[0] == 0.123 && r2v[0] == 0.017 && r2v[1] == y, "an insert and a delete at one tail");
}

static uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
static double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

struct Graph {
    std::vector<int> ptr, tail, d;
};
static bool read_graph(FILE *f, int V, Graph &g) {
    int E = 0;
    if (std::fscanf(f, "%d", &E) != 1 || E < 0) return false;
    g.ptr.assign((size_t)V + 1, 0);
    g.tail.assign((size_t)E, 0);
    g.d.assign((size_t)V, 0);
    for (int &x : g.ptr)
        if (std::fscanf(f, "%d", &x) != 1) return false;
    for (int &x : g.tail)
        if (std::fscanf(f, "%d", &x) != 1) return false;
    for (int &x : g.d)
        if (std::fscanf(f, "%d", &x) != 1) return false;
    return g.ptr[(size_t)V] == E;
}

struct Column {
    double eps = 0.0;
    std::vector<int> ids;
    std::vector<double> w, p, r;
};

static void rounds_and_print(int step, int ci, int V, const Graph &g, Column &c, int max_rounds, int piece, const long long *fix,
                             const std::vector<int> *rowless = nullptr) {
    std::vector<double> y((size_t)V, 0.0);
    long long pushes = 0;
    int used = 0;
    for (int k = 0; k < max_rounds; ++k) {
        const long long n = ft_round_ref(V, g.ptr.data(), g.tail.data(), g.d.data(), c.eps, c.p.data(), c.r.data(), y.data(), piece);
        if (!n) break;
        pushes += n;
        ++used;
    }
    long long left = 0;
    for (int u = 0; u < V; ++u) {
        volatile double thr = c.eps * (double)(g.d[(size_t)u] + 1);
        left += std::fabs(c.r[(size_t)u]) > thr ? 1 : 0;
    }
    if (rowless) // settled exactly: no round, no statistic
        for (int j : *rowless) c.p[(size_t)c.ids[(size_t)j]] = fp_rowless_p(c.w[(size_t)j]);
    std::printf("state %d %d %d %lld %lld %lld %lld %lld", step, ci, used, pushes, left, fix[0], fix[1], fix[2]);
    for (int u = 0; u < V; ++u) std::printf(" %016" PRIx64 " %016" PRIx64, bits_of(c.p[(size_t)u]), bits_of(c.r[(size_t)u]));
    std::printf("\n");
}

static bool run_case(const char *path) {
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    int V = 0, n_cols = 0, n_steps = 0, rounds0 = 0;
    bool ok = std::fscanf(f, "%d %d %d %d", &V, &n_cols, &n_steps, &rounds0) == 4 && V > 0 && n_cols > 0;
    std::vector<Column> cols((size_t)(ok ? n_cols : 0));
    for (Column &c : cols) {
        int n = 0;
        uint64_t b = 0;
        ok = ok && std::fscanf(f, "%" SCNx64 " %d", &b, &n) == 2 && n > 0;
        if (!ok) break;
        c.eps = from_bits(b);
        c.ids.assign((size_t)n, 0);
        c.w.assign((size_t)n, 0.0);
        for (int j = 0; j < n && ok; ++j) {
            ok = std::fscanf(f, "%d %" SCNx64, &c.ids[(size_t)j], &b) == 2 && c.ids[(size_t)j] >= 0 && c.ids[(size_t)j] < V;
            c.w[(size_t)j] = from_bits(b);
        }
    }
    Graph g;
    ok = ok && read_graph(f, V, g);
    const long long none[3] = {0, 0, 0};
    for (size_t ci = 0; ok && ci < cols.size(); ++ci) { // create
        Column &c = cols[ci];
        c.p.assign((size_t)V, 0.0);
        c.r.assign((size_t)V, 0.0);
        std::vector<int> rowless;
        for (size_t j = 0; j < c.ids.size(); ++j) {
            const int q = c.ids[j];
            if (g.ptr[(size_t)q + 1] == g.ptr[(size_t)q] && g.d[(size_t)q] == 0) rowless.push_back((int)j);
            else c.r[(size_t)q] = c.w[j];
        }
        rounds_and_print(0, (int)ci, V, g, c, rounds0, ci % 2 ? 64 : fw_piece(0), none, &rowless);
    }
    for (int s = 1; ok && s <= n_steps; ++s) {
        int kind = 0, max_rounds = 0;
        ok = std::fscanf(f, "%d %d", &kind, &max_rounds) == 2 && max_rounds >= 1;
        if (!ok) break;
        std::vector<int> tail, head;
        std::vector<unsigned char> ins;
        if (kind == 1) {
            int L = 0;
            ok = std::fscanf(f, "%d", &L) == 1 && L >= 0;
            tail.assign((size_t)(ok ? L : 0), 0);
            head = tail;
            ins.assign(tail.size(), 0);
            for (size_t i = 0; ok && i < tail.size(); ++i) {
                int x = 0;
                ok = std::fscanf(f, "%d %d %d", &tail[i], &head[i], &x) == 3;
                ins[i] = (unsigned char)x;
            }
            ok = ok && read_graph(f, V, g);
        }
        for (size_t ci = 0; ok && ci < cols.size(); ++ci) {
            long long fix[3] = {0, 0, 0};
            if (kind == 1)
                ft_fixup_ref(V, cols[ci].p.data(), cols[ci].r.data(), g.d.data(), (int)tail.size(), tail.data(), head.data(), ins.data(), fix);
            rounds_and_print(s, (int)ci, V, g, cols[ci], max_rounds, (s + (int)ci) % 2 ? 64 : fw_piece(0), fix);
        }
    }
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv) {
    plan();
    by_hand();
    if (argc > 1) CHECK(run_case(argv[1]), "the case file %s", argv[1]);
    std::printf("ftrack_plan_test: %d failures\n", failures);
    return failures ? 1 : 0;
}
