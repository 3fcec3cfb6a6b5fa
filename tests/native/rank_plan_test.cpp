// rank_plan_test.cpp -- dynamicppr_amd/csrc/dppr_rank_plan.hpp on the CPU: every rejection of the spec and of a call's arguments
// at its limit, which specs need the epoch, the flat seed list of source and set lanes, the piece list against a brute-force split
// (rows of length 0, 1, piece, piece + 1, a seed repeated across lanes, every flag combination), its bound, and the scratch sizes.
// Every array is exactly as long as the code may touch (the sanitizers watch the bounds).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_rank_plan.hpp"

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

static dppr_rank_spec_t spec_of(int factor, int dtype, int mask, uint32_t exclude) {
    dppr_rank_spec_t s{};
    s.factor = factor;
    s.factor_dtype = dtype;
    s.mask = mask;
    s.exclude = exclude;
    return s;
}

static void specs() {
    CHECK(rank_spec_ok(nullptr) && !rank_needs_epoch(nullptr) && !rank_needs_factor_dev(nullptr) && !rank_needs_mask_dev(nullptr), "NULL is the zero spec");
    for (int f = -1; f <= 4; ++f)
        for (int m = -1; m <= 3; ++m) {
            const dppr_rank_spec_t s = spec_of(f, DPPR_F64, m, 0);
            const bool want = f >= 0 && f <= 3 && m >= 0 && m <= 2;
            CHECK(rank_spec_ok(&s) == want, "factor %d mask %d", f, m);
        }
    for (int dt = -1; dt <= 2; ++dt) {
        const dppr_rank_spec_t dev = spec_of(DPPR_FACTOR_DEV, dt, 0, 0), deg = spec_of(DPPR_FACTOR_DEG, dt, 0, 0);
        CHECK(rank_spec_ok(&dev) == (dt == DPPR_F64 || dt == DPPR_F32), "dtype %d is read for DEV", dt);
        CHECK(rank_spec_ok(&deg), "dtype %d is not read for DEG", dt);
    }
    for (uint32_t x = 0; x < 8; ++x) {
        const dppr_rank_spec_t s = spec_of(0, 0, 0, x);
        CHECK(rank_spec_ok(&s), "exclude %u", x);
        CHECK(rank_needs_epoch(&s) == ((x & 6u) != 0), "exclude %u and the epoch", x);
    }
    for (uint32_t x : {8u, 9u, 0x80000000u, 0xfffffff8u}) {
        const dppr_rank_spec_t s = spec_of(0, 0, 0, x);
        CHECK(!rank_spec_ok(&s), "unknown exclude bits %u", x);
    }
    for (int f = 0; f <= 3; ++f) {
        const dppr_rank_spec_t s = spec_of(f, 0, DPPR_MASK_ALLOW, DPPR_EXCLUDE_SEEDS);
        CHECK(rank_needs_epoch(&s) == (f == DPPR_FACTOR_DEG || f == DPPR_FACTOR_INV_DEG), "factor %d and the epoch", f);
        CHECK(rank_needs_factor_dev(&s) == (f == DPPR_FACTOR_DEV) && rank_needs_mask_dev(&s), "factor %d and the pointers", f);
    }
    // what the kernels read of a spec: pointers only where their kind asks for them
    int dummy = 0;
    dppr_rank_spec_t s = spec_of(DPPR_FACTOR_DEG, DPPR_F32, DPPR_MASK_NONE, 5);
    s.factor_dev = &dummy;
    s.mask_dev = reinterpret_cast<const uint8_t *>(&dummy);
    RkSpec r = rank_spec(&s);
    CHECK(r.factor == DPPR_FACTOR_DEG && !r.factor_dev && !r.mask_dev && r.exclude == 5, "DEG without a mask reads no pointer");
    s.factor = DPPR_FACTOR_DEV;
    s.mask = DPPR_MASK_DENY;
    r = rank_spec(&s);
    CHECK(r.factor_dev == &dummy && r.mask_dev && r.factor_dtype == DPPR_F32 && r.mask == DPPR_MASK_DENY, "DEV with a mask reads both");
    r = rank_spec(nullptr);
    CHECK(r.factor == 0 && r.mask == 0 && r.exclude == 0 && !r.factor_dev && !r.mask_dev, "NULL");
    CHECK(rank_factor_bytes(DPPR_F64, 1000) == 8000 && rank_factor_bytes(DPPR_F32, 1000) == 4000 && rank_mask_bytes(1000) == 1000 &&
              rank_factor_elem_bytes(DPPR_F32) == 4 && rank_factor_elem_bytes(DPPR_F64) == 8,
          "bytes of the caller's vectors");
}

static void arguments() {
    int32_t ids[2] = {0, 99}, cnt = 0;
    double sc = 0;
    const dppr_rank_spec_t good = spec_of(DPPR_FACTOR_INV_DEG, 0, DPPR_MASK_DENY, 7), bad = spec_of(4, 0, 0, 0);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(rank_topk_args_ok(&good, 1, 0.0, ids, &sc, &cnt) && rank_topk_args_ok(nullptr, DPPR_TOPK_MAX, inf, ids, &sc, &cnt), "valid");
    CHECK(!rank_topk_args_ok(&bad, 1, 0.0, ids, &sc, &cnt), "a bad spec");
    CHECK(!rank_topk_args_ok(&good, 0, 0.0, ids, &sc, &cnt) && !rank_topk_args_ok(&good, DPPR_TOPK_MAX + 1, 0.0, ids, &sc, &cnt) &&
              !rank_topk_args_ok(&good, -1, 0.0, ids, &sc, &cnt),
          "k");
    CHECK(!rank_topk_args_ok(&good, 1, -1e-300, ids, &sc, &cnt) && !rank_topk_args_ok(&good, 1, nan, ids, &sc, &cnt) &&
              rank_topk_args_ok(&good, 1, -0.0, ids, &sc, &cnt),
          "min_score");
    CHECK(!rank_topk_args_ok(&good, 1, 0.0, nullptr, &sc, &cnt) && !rank_topk_args_ok(&good, 1, 0.0, ids, nullptr, &cnt) &&
              !rank_topk_args_ok(&good, 1, 0.0, ids, &sc, nullptr),
          "NULL outputs");
    CHECK(rank_score_at_args_ok(&good, ids, 2, 100, &sc) && rank_score_at_args_ok(nullptr, nullptr, 0, 100, &sc), "valid score_at, m == 0");
    CHECK(!rank_score_at_args_ok(&good, ids, 2, 99, &sc) && !rank_score_at_args_ok(&good, ids, -1, 100, &sc) &&
              !rank_score_at_args_ok(&good, nullptr, 2, 100, &sc) && !rank_score_at_args_ok(&good, ids, 2, 100, nullptr) &&
              !rank_score_at_args_ok(&bad, ids, 2, 100, &sc),
          "score_at");
    const int32_t neg[1] = {-1};
    CHECK(!rank_score_at_args_ok(&good, neg, 1, 100, &sc), "a negative id");
    CHECK(rank_piece_ok(1) && rank_piece_ok(RK_PIECE) && !rank_piece_ok(0) && !rank_piece_ok(RK_PIECE + 1) && !rank_piece_ok(-5), "piece");
}

static void seeds() {
    // a slot
    const int one[1] = {42};
    RkSeeds s = rk_seeds(one, nullptr, 1);
    CHECK(s.n == 1 && s.total() == 1 && s.off[1] == 1 && s.off[Q_LANES] == 1 && rk_lane_of(s, 0) == 0, "a slot");
    // a source group of 16
    int src[Q_LANES];
    for (int i = 0; i < Q_LANES; ++i) src[i] = 100 + i;
    s = rk_seeds(src, nullptr, Q_LANES);
    CHECK(s.total() == Q_LANES, "16 sources");
    for (int i = 0; i < Q_LANES; ++i) CHECK(rk_lane_of(s, i) == i, "lane of source %d", i);
    // a target group: lanes of 1 (a source lane), 2, 40 and 300 seeds; the table lists the source lane's seed too
    const int mixed[4] = {7, -1, -1, -1};
    int tg_off[Q_LANES + 1] = {0, 1, 3, 43, 343};
    for (int i = 5; i <= Q_LANES; ++i) tg_off[i] = 343;
    s = rk_seeds(mixed, tg_off, 4);
    CHECK(s.total() == 343 && s.off[1] == 1 && s.off[2] == 3 && s.off[3] == 43 && s.off[4] == 343, "set lanes");
    const int at[] = {0, 1, 2, 3, 42, 43, 342}, lane[] = {0, 1, 1, 2, 2, 3, 3};
    for (int i = 0; i < 7; ++i) CHECK(rk_lane_of(s, at[i]) == lane[i], "lane of position %d", at[i]);
    // a set lane without a table holds nothing (never built by the engine; the plan must not read past it)
    const int none[2] = {-1, 3};
    s = rk_seeds(none, nullptr, 2);
    CHECK(s.total() == 1 && s.off[1] == 0 && rk_lane_of(s, 0) == 1, "an empty lane before a source lane");
}

// the definition: piece c of a row of len entries covers [c * piece, min(len, (c + 1) * piece))
static void brute(const std::vector<int> &len, uint32_t exclude, int piece, std::multiset<unsigned long long> &out, long long *covered) {
    for (size_t pos = 0; pos < len.size() / 2; ++pos)
        for (unsigned dir = 0; dir < 2; ++dir) {
            if (!(exclude & (dir ? DPPR_EXCLUDE_IN_NEIGHBOURS : DPPR_EXCLUDE_OUT_NEIGHBOURS))) continue;
            for (long long lo = 0, c = 0; lo < len[2 * pos + dir]; lo += piece, ++c) {
                out.insert(((unsigned long long)pos << 32) | ((unsigned long long)dir << 31) | (unsigned long long)c);
                *covered += std::min<long long>(piece, len[2 * pos + dir] - lo);
            }
        }
}

static void pieces() {
    std::vector<unsigned long long> got;
    for (int piece : {1, 3, 64, RK_PIECE}) {
        // seeds: rows of 0, 1, piece, piece + 1, 3 piece - 1 entries, and the first seed again as the seed of a second lane
        const std::vector<int> len = {0, 1, 1, 0, piece, piece + 1, piece + 1, piece, 3 * piece - 1, 2 * piece, 0, 1};
        const int total = (int)len.size() / 2;
        for (uint32_t x = 0; x < 8; ++x) {
            rk_pieces(len.data(), total, x, piece, got);
            std::multiset<unsigned long long> want;
            long long covered = 0, sum = 0;
            brute(len, x, piece, want, &covered);
            for (int pos = 0; pos < total; ++pos) sum += ((x & 4u) ? len[2 * pos] : 0) + ((x & 2u) ? len[2 * pos + 1] : 0);
            CHECK(std::multiset<unsigned long long>(got.begin(), got.end()) == want && covered == sum, "piece %d exclude %u", piece, x);
            CHECK(std::set<unsigned long long>(got.begin(), got.end()).size() == got.size(), "no piece twice (piece %d exclude %u)", piece, x);
            for (unsigned long long it : got) {
                const int l = len[2 * cl_item_pos(it) + cl_item_dir(it)];
                CHECK((long long)cl_item_chunk(it) * piece < l, "a piece past its row");
            }
            if (!(x & 6u)) CHECK(got.empty(), "SEEDS alone walks no row");
        }
        // the exact counts of the limits
        rk_pieces(len.data(), total, DPPR_EXCLUDE_OUT_NEIGHBOURS, piece, got);
        CHECK((long long)got.size() == 0 + 1 + 1 + 2 + (piece > 1 ? 3 : 2) + 0, "out-rows: 0, 1, piece, piece + 1, 3 piece - 1, 0 (piece %d: %zu)", piece, got.size());
        rk_pieces(len.data(), total, DPPR_EXCLUDE_IN_NEIGHBOURS, piece, got);
        CHECK((long long)got.size() == 1 + 0 + 2 + 1 + 2 + 1, "in-rows (piece %d: %zu)", piece, got.size());
    }
    rk_pieces(nullptr, 0, 7, 64, got);
    CHECK(got.empty(), "no seeds");
    // the bound: random lanes of distinct seeds over a random graph never have more pieces than rk_piece_cap says
    std::mt19937 rng(7);
    for (int round = 0; round < 200; ++round) {
        const int V = 1 + (int)(rng() % 60), piece = 1 + (int)(rng() % 9), n = 1 + (int)(rng() % Q_LANES);
        std::vector<int> outdeg((size_t)V, 0), indeg((size_t)V, 0);
        const long long Ed = rng() % 400;
        for (long long i = 0; i < Ed; ++i) {
            ++outdeg[rng() % (size_t)V];
            ++indeg[rng() % (size_t)V];
        }
        int src[Q_LANES], tg_off[Q_LANES + 1] = {0};
        std::vector<int> len;
        for (int i = 0; i < Q_LANES; ++i) {
            src[i] = -1;
            int m = 0;
            if (i < n) {
                m = 1 + (int)(rng() % (size_t)V);
                std::vector<int> perm((size_t)V);
                for (int v = 0; v < V; ++v) perm[(size_t)v] = v;
                std::shuffle(perm.begin(), perm.end(), rng);
                if (m == 1 && (rng() & 1)) src[i] = perm[0]; // (a source lane: the table still lists its seed)
                for (int j = 0; j < m; ++j) {
                    len.push_back(outdeg[(size_t)perm[(size_t)j]]);
                    len.push_back(indeg[(size_t)perm[(size_t)j]]);
                }
            }
            tg_off[i + 1] = tg_off[i] + m;
        }
        const RkSeeds s = rk_seeds(src, tg_off, n);
        CHECK(s.total() == tg_off[Q_LANES], "flat list");
        for (uint32_t x : {2u, 4u, 6u, 7u, 1u}) {
            rk_pieces(len.data(), s.total(), x, piece, got);
            CHECK(got.size() <= rk_piece_cap(s, Ed, x, piece), "bound: %zu pieces, cap %zu (V %d Ed %lld piece %d n %d exclude %u)", got.size(),
                  rk_piece_cap(s, Ed, x, piece), V, Ed, piece, n, x);
        }
        CHECK(rk_piece_cap(s, Ed, DPPR_EXCLUDE_SEEDS, piece) == 0, "SEEDS alone needs no list");
    }
}

static void scratch() {
    CHECK(rk_excl_elems(0) == 1 && rk_excl_elems(4096) == 4096 && rk_len_elems(0) == 2 && rk_len_elems(343) == 686, "marking");
    CHECK(rk_chunks(0, 512) == 0 && rk_chunks(1, 512) == 1 && rk_chunks(512, 512) == 1 && rk_chunks(513, 512) == 2, "chunks");
}

int main() {
    specs();
    arguments();
    seeds();
    pieces();
    scratch();
    std::printf("rank plan: %d failures\n", failures);
    return failures ? 1 : 0;
}
