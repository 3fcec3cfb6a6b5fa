// assign_plan_test.cpp -- dynamicppr_amd/csrc/dppr_assign_plan.hpp on the CPU: the class table of a call, the team that reads a
// vertex, tile counts and the workspace, the result block (sections aligned, in order, disjoint, inside the block; written whole
// into a buffer of exactly total_bytes: the sanitizers watch the bounds) for C in {1, 16, 17, 256} classes of counts, and every
// argument rule of both calls against a plain restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_assign_plan.hpp"

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
    static_assert(DPPR_ASSIGN_GROUPS_MAX == 16 && DPPR_ASSIGN_CLASSES_MAX == 256, "the limits of include/dppr.h");
    static_assert(AS_HEAD_BYTES == 2072 && AS_HEAD_BYTES % 8 == 0, "the sections start aligned");
    static_assert(offsetof(AsHead, n_flips) == 0 && offsetof(AsHead, go) == 8 && offsetof(AsHead, counts) == 16, "the head");
    static_assert(sizeof(AsGroup) == 24 && sizeof(AsDesc) == 16 * 24 + 8, "the descriptors travel as a kernel argument");
    // tiles and workspace
    for (int64_t V : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)777, (int64_t)1 << 22}) {
        ++cases;
        int64_t want = 0;
        for (int64_t v = 0; v < V; v += 256) ++want;
        CHECK(as_tiles(V) == want, "V %lld", (long long)V);
        const AsWork w = as_workspace(V);
        CHECK(w.cnt_elems == (size_t)want && w.base_elems == (size_t)want && w.ws_plane == (size_t)want * 256 && w.ws_elems == 3 * w.ws_plane,
              "V %lld", (long long)V);
        CHECK(w.ws_plane >= (size_t)V && w.scale_elems == 256, "a plane holds every id: V %lld", (long long)V);
        CHECK(w.bytes == 4 * (2 * (size_t)want + 768 * (size_t)want) + 2048, "V %lld", (long long)V);
    }
    CHECK(as_tiles(1) == 1 && as_tiles(255) == 1 && as_tiles(256) == 1 && as_tiles(257) == 2, "the tile counts at the edges");
    CHECK(as_workspace(0).cnt_elems == 1, "a workspace is never empty");
    CHECK(as_tiles(((int64_t)1 << 31) + 5) == ((int64_t)1 << 23) + 1, "tile count past 2^31 ids");
    // the team: one step of 16-byte pieces over the widest row
    {
        const int want[17] = {1, 1, 1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8, 8, 8};
        for (int gw = 1; gw <= 16; ++gw) {
            ++cases;
            const int t = as_team(gw);
            CHECK(t == want[gw], "gw %d: team %d", gw, t);
            CHECK(256 % t == 0 && (2 * t >= gw || t == AS_TEAM_MAX), "gw %d", gw);
        }
    }
    // the class table
    {
        const int one[1] = {1}, sixteen[1] = {16}, mix[3] = {16, 1, 5};
        AsTable t = as_table(one, 1);
        CHECK(t.ok && t.C == 1 && t.base[0] == 0, "C = 1");
        t = as_table(sixteen, 1);
        CHECK(t.ok && t.C == 16, "C = 16");
        const int sev[2] = {16, 1};
        t = as_table(sev, 2);
        CHECK(t.ok && t.C == 17 && t.base[1] == 16, "C = 17");
        t = as_table(mix, 3);
        CHECK(t.ok && t.C == 22 && t.base[0] == 0 && t.base[1] == 16 && t.base[2] == 17, "bases in call order");
        int full[16];
        for (int &x : full) x = 16;
        t = as_table(full, 16);
        CHECK(t.ok && t.C == 256 && t.base[15] == 240, "C = 256");
        CHECK(!as_table(full, 17).ok && !as_table(full, 0).ok && !as_table(full, -1).ok && !as_table(nullptr, 1).ok, "n_groups out of range");
        const int zero[2] = {3, 0}, wide[2] = {3, 17};
        CHECK(!as_table(zero, 2).ok && !as_table(wide, 2).ok, "a lane count outside [1, 16]");
        cases += 8;
    }
    // the block: for C classes of counts, V ids, cap flips
    for (int C : {1, 16, 17, 256})
        for (int64_t V : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257})
            for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)257})
                for (int flags = 0; flags < 8; ++flags) {
                    ++cases;
                    const bool wb = flags & 1, wm = flags & 2, host = flags & 4;
                    const int64_t capc = as_cap_clamped(cap, V);
                    CHECK(capc == (cap < V ? cap : V), "cap clamps to V");
                    const AsLayout l = as_layout(V, capc, wb, wm, host);
                    const size_t v = host ? (size_t)V : 0, c = host ? (size_t)capc : 0;
                    if (!host) CHECK(l.total_bytes == AS_HEAD_BYTES, "a device destination is the head alone");
                    CHECK(l.off_label == AS_HEAD_BYTES, "label first");
                    CHECK(l.off_best >= l.off_label + 4 * v && l.off_best < l.off_label + 4 * v + 8, "V %lld", (long long)V);
                    CHECK(l.off_margin == l.off_best + (wb ? 8 * v : 0) && l.off_fid == l.off_margin + (wm ? 8 * v : 0), "V %lld", (long long)V);
                    CHECK(l.off_fold >= l.off_fid + 4 * c && l.off_fnew >= l.off_fold + 4 * c && l.total_bytes >= l.off_fnew + 4 * c, "cap %lld", (long long)cap);
                    CHECK(l.total_bytes < l.off_fid + 12 * c + 24, "no more than the padding");
                    for (size_t off : {l.off_label, l.off_best, l.off_margin, l.off_fid, l.off_fold, l.off_fnew, l.total_bytes})
                        CHECK(off % 8 == 0, "aligned: %zu", off);
                    // written whole, read back: nothing overlaps, nothing lies outside
                    std::vector<unsigned char> block(l.total_bytes, 0xEE);
                    AsHead head;
                    std::memset(&head, 0, sizeof(head));
                    head.n_flips = 77, head.go = 1;
                    for (int i = 0; i <= C; ++i) head.counts[i] = 1000 + i;
                    std::vector<int32_t> lab(v, 3), fi(c, 4), fo(c, 5), fn(c, 6);
                    std::vector<double> b(v, 7.0), m(v, 8.0);
                    std::memcpy(block.data(), &head, sizeof(head));
                    if (v) std::memcpy(block.data() + l.off_label, lab.data(), 4 * v);
                    if (v && wb) std::memcpy(block.data() + l.off_best, b.data(), 8 * v);
                    if (v && wm) std::memcpy(block.data() + l.off_margin, m.data(), 8 * v);
                    if (c) std::memcpy(block.data() + l.off_fid, fi.data(), 4 * c);
                    if (c) std::memcpy(block.data() + l.off_fold, fo.data(), 4 * c);
                    if (c) std::memcpy(block.data() + l.off_fnew, fn.data(), 4 * c);
                    AsHead h2;
                    std::vector<int32_t> lab2(v), fi2(c), fo2(c), fn2(c);
                    std::vector<double> b2(v, 7.0), m2(v, 8.0);
                    std::memcpy(&h2, block.data(), sizeof(h2));
                    if (v) std::memcpy(lab2.data(), block.data() + l.off_label, 4 * v);
                    if (v && wb) std::memcpy(b2.data(), block.data() + l.off_best, 8 * v);
                    if (v && wm) std::memcpy(m2.data(), block.data() + l.off_margin, 8 * v);
                    if (c) std::memcpy(fi2.data(), block.data() + l.off_fid, 4 * c);
                    if (c) std::memcpy(fo2.data(), block.data() + l.off_fold, 4 * c);
                    if (c) std::memcpy(fn2.data(), block.data() + l.off_fnew, 4 * c);
                    bool same = lab2 == lab && b2 == b && m2 == m && fi2 == fi && fo2 == fo && fn2 == fn && h2.n_flips == 77 && h2.go == 1;
                    for (int i = 0; i <= C; ++i) same = same && h2.counts[i] == 1000 + i;
                    CHECK(same, "sections overlap: C %d V %lld cap %lld flags %d", C, (long long)V, (long long)cap, flags);
                }
    CHECK(as_layout(-3, -5, true, true, true).total_bytes == AS_HEAD_BYTES, "negative sizes are the head alone");
    // the argument rules, each at its limit
    int x = 0;
    const void *some = &x;
    const int32_t gs[16] = {0};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double mm[] = {-inf, -1.0, -1e-300, -0.0, 0.0, 1e-300, 0.5, 1e300, inf, nan};
    const int64_t cc[] = {std::numeric_limits<int64_t>::min(), -1, 0, 1, 1000, std::numeric_limits<int64_t>::max()};
    for (int ng : {-1, 0, 1, 16, 17})
        for (int has_g = 0; has_g < 2; ++has_g)
            for (double m : mm)
                for (int dest = -1; dest <= 2; ++dest)
                    for (int64_t cap : cc)
                        for (int mask = 0; mask < 32; ++mask) {
                            ++cases;
                            const void *ol = mask & 1 ? some : nullptr, *oc = mask & 2 ? some : nullptr, *fi = mask & 4 ? some : nullptr;
                            const void *fo = mask & 8 ? some : nullptr, *fn = mask & 16 ? some : nullptr;
                            AsCheck want = AS_OK;
                            if (!has_g || ng < 1 || ng > 16) want = AS_BAD_GROUPS;
                            else if (std::isnan(m) || m < 0.0) want = AS_BAD_MIN;
                            else if (dest != 0 && dest != 1) want = AS_BAD_DEST;
                            else if (!ol || !oc) want = AS_NULL_OUT;
                            else if (cap < 0 || (cap > 0 && !(fi && fo && fn))) want = AS_BAD_CAP;
                            const AsCheck got = as_check(has_g ? gs : nullptr, ng, m, dest, ol, oc, cap, fi, fo, fn);
                            CHECK(got == want, "ng %d g %d m %g dest %d cap %lld mask %d: %d, want %d", ng, has_g, m, dest, (long long)cap, mask, got, want);
                        }
    {
        const int32_t in[3] = {0, 5, 9}, low[2] = {0, -1}, high[2] = {10, 0};
        CHECK(as_at_check(gs, 1, 0.0, in, 3, 10, some) == AS_OK, "ids inside");
        CHECK(as_at_check(gs, 1, 0.0, nullptr, 0, 10, some) == AS_OK, "m = 0 needs no ids");
        CHECK(as_at_check(gs, 1, 0.0, nullptr, 1, 10, some) == AS_BAD_IDS && as_at_check(gs, 1, 0.0, in, -1, 10, some) == AS_BAD_IDS, "NULL ids, m < 0");
        CHECK(as_at_check(gs, 1, 0.0, low, 2, 10, some) == AS_BAD_IDS && as_at_check(gs, 1, 0.0, high, 2, 10, some) == AS_BAD_IDS, "an id outside");
        CHECK(as_at_check(gs, 1, 0.0, in, 3, 10, nullptr) == AS_NULL_OUT, "NULL out_label");
        CHECK(as_at_check(gs, 0, 0.0, in, 3, 10, some) == AS_BAD_GROUPS && as_at_check(gs, 17, 0.0, in, 3, 10, some) == AS_BAD_GROUPS, "n_groups");
        CHECK(as_at_check(gs, 1, -1e-300, in, 3, 10, some) == AS_BAD_MIN && as_at_check(gs, 1, nan, in, 3, 10, some) == AS_BAD_MIN, "min_score");
        cases += 7;
    }
    {
        const double ok[4] = {0.0, 1.0, 1e300, 5e-324}, neg[2] = {1.0, -1e-300}, bad_inf[2] = {inf, 1.0}, bad_nan[3] = {1.0, 1.0, nan};
        const double mz[1] = {-0.0};
        CHECK(as_scale_ok(nullptr, 256) && as_scale_ok(ok, 4) && as_scale_ok(mz, 1), "NULL, finite and >= 0 (-0.0 compares equal to 0)");
        CHECK(!as_scale_ok(neg, 2) && !as_scale_ok(bad_inf, 2) && !as_scale_ok(bad_nan, 3), "negative, infinite, NaN");
        CHECK(as_scale_ok(bad_nan, 2), "only the C entries of the call are read");
        cases += 3;
    }
    for (int c = AS_OK; c <= AS_BAD_IDS; ++c) CHECK(std::strlen(as_check_text((AsCheck)c)) > 1, "every rule has its words");
    std::printf("assign_plan_test: %ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
