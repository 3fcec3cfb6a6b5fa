// patch_plan_test.cpp -- dynamicppr_amd/csrc/dppr_patch_plan.hpp on the CPU: the workspace, the block of a patch to the host
// (sections aligned, in order, disjoint, inside the block; written whole into a buffer of exactly total_bytes: the sanitizers
// watch the bounds) at caps of 0, 1 and odd counts, and every argument check at its limit against a plain restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_patch_plan.hpp"

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
    static_assert(PT_HEAD_BYTES == 280 && PT_HEAD_BYTES % 8 == 0, "the sections start aligned");
    static_assert(DPPR_PATCH_KEEP_MARK == 0 && DPPR_PATCH_REMARK_ALL == 1 && DPPR_PATCH_REMARK_EMITTED == 2, "the modes");
    // workspace
    for (int64_t V : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)1 << 22, ((int64_t)1 << 31) + 5}) {
        ++cases;
        int64_t tiles = 0;
        for (int64_t v = 0; v < V; v += EX_TILE) ++tiles;
        const PtWork w = pt_workspace(V);
        CHECK(w.mask_elems == (size_t)V && w.cnt_elems == (size_t)tiles * 32 && w.base_elems == (size_t)tiles * 32, "V %lld", (long long)V);
        CHECK(w.bytes == 4 * (size_t)V + 384 * (size_t)tiles, "V %lld", (long long)V);
    }
    CHECK(pt_workspace(0).mask_elems == 1 && pt_workspace(0).cnt_elems == 32, "an empty id space still has buffers");
    // the block
    const int64_t caps[] = {0, 1, 2, 3, 7, 8, 255, 257, 100003};
    for (int64_t cu : caps)
        for (int64_t cd : caps) {
            ++cases;
            const PtLayout l = pt_layout(cu, cd);
            const size_t u = (size_t)cu, d = (size_t)cd;
            CHECK(l.off_up_ids == PT_HEAD_BYTES, "caps %lld %lld", (long long)cu, (long long)cd);
            CHECK(l.off_up_p >= l.off_up_ids + 4 * u && l.off_up_p < l.off_up_ids + 4 * u + 8 && l.off_up_p % 8 == 0, "caps %lld %lld", (long long)cu, (long long)cd);
            CHECK(l.off_del_ids == l.off_up_p + 8 * u && l.off_del_ids % 8 == 0, "caps %lld %lld", (long long)cu, (long long)cd);
            CHECK(l.total_bytes >= l.off_del_ids + 4 * d && l.total_bytes < l.off_del_ids + 4 * d + 8 && l.total_bytes % 8 == 0, "caps %lld %lld", (long long)cu, (long long)cd);
            std::vector<unsigned char> block(l.total_bytes, 0xEE);
            PtHead head;
            for (int i = 0; i <= PT_LANES; ++i) {
                head.up_offsets[i] = 1000 + i;
                head.del_offsets[i] = 2000 + i;
            }
            head.go = 1;
            head.written = 1;
            std::vector<int32_t> ui(u, 3), di(d, 4);
            std::vector<double> up(u, 5.0);
            std::memcpy(block.data(), &head, sizeof(head));
            if (u) std::memcpy(block.data() + l.off_up_ids, ui.data(), 4 * u);
            if (u) std::memcpy(block.data() + l.off_up_p, up.data(), 8 * u);
            if (d) std::memcpy(block.data() + l.off_del_ids, di.data(), 4 * d);
            PtHead h2;
            std::vector<int32_t> ui2(u), di2(d);
            std::vector<double> up2(u);
            std::memcpy(&h2, block.data(), sizeof(h2));
            if (u) std::memcpy(ui2.data(), block.data() + l.off_up_ids, 4 * u);
            if (u) std::memcpy(up2.data(), block.data() + l.off_up_p, 8 * u);
            if (d) std::memcpy(di2.data(), block.data() + l.off_del_ids, 4 * d);
            bool same = ui2 == ui && up2 == up && di2 == di && h2.go == 1 && h2.written == 1;
            for (int i = 0; i <= PT_LANES; ++i) same = same && h2.up_offsets[i] == 1000 + i && h2.del_offsets[i] == 2000 + i;
            CHECK(same, "sections overlap: caps %lld %lld", (long long)cu, (long long)cd);
        }
    CHECK(pt_layout(-5, -1).total_bytes == PT_HEAD_BYTES && pt_layout(0, 0).total_bytes == PT_HEAD_BYTES, "no caps: the head alone");
    {
        ++cases;
        const int64_t big = 16 * (((int64_t)1 << 28) + 3);
        const PtLayout l = pt_layout(big, big);
        CHECK(l.off_del_ids == PT_HEAD_BYTES + 12 * (size_t)big && l.total_bytes == l.off_del_ids + 4 * (size_t)big, "a block past 2^36 bytes");
    }
    // the argument checks
    int64_t off[2] = {0, 0};
    int32_t ids[1] = {0};
    double pv[1] = {0.0};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double mm[] = {-inf, -1.0, -1e-300, -std::numeric_limits<double>::denorm_min(), -0.0, 0.0, std::numeric_limits<double>::denorm_min(), 1e-9, 1.0, inf, nan};
    const int64_t cc[] = {std::numeric_limits<int64_t>::min(), -1, 0, 1, std::numeric_limits<int64_t>::max()};
    auto ok_value = [](double m) { return !std::isnan(m) && !(m < 0.0); };
    for (double tau : mm)
        for (double delta : mm)
            for (int64_t cu : cc)
                for (int64_t cd : cc)
                    for (int dest = -1; dest <= 2; ++dest)
                        for (int remark = -1; remark <= 3; ++remark)
                            for (int mask = 0; mask < 32; ++mask) {
                                ++cases;
                                dppr_patch_out_t out;
                                out.up_offsets = mask & 1 ? off : nullptr;
                                out.del_offsets = mask & 2 ? off : nullptr;
                                out.up_ids = mask & 4 ? ids : nullptr;
                                out.up_p = mask & 8 ? pv : nullptr;
                                out.del_ids = mask & 16 ? ids : nullptr;
                                out.written = 77;
                                const bool want = ok_value(tau) && ok_value(delta) && cu >= 0 && cd >= 0 && (dest == 0 || dest == 1) &&
                                                  remark >= 0 && remark <= 2 && out.up_offsets && out.del_offsets &&
                                                  (cu == 0 || (out.up_ids && out.up_p)) && (cd == 0 || out.del_ids);
                                CHECK(pt_args_ok(tau, delta, cu, cd, dest, remark, &out) == want,
                                      "tau %g delta %g caps %lld %lld dest %d remark %d mask %d", tau, delta, (long long)cu, (long long)cd, dest, remark, mask);
                                CHECK(out.written == 77, "a check writes nothing");
                            }
    CHECK(!pt_args_ok(0.0, 0.0, 0, 0, 0, 0, nullptr), "a NULL out");
    std::printf("patch_plan_test: %ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
