// CPU test driver for dynamicppr_amd/csrc/dppr_devbuf.hpp (the owner type of the engine's device and pinned memory), with a host
// allocator policy that counts live bytes and blocks, logs its calls and can be told to fail the n-th allocation. Built with
// ASan + UBSan: a double free, a use after free or a leak ends the run whatever the counters say.   devbuf_test <seed> <cases>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../dynamicppr_amd/csrc/dppr_devbuf.hpp"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 10) { printf("FAILED %s (line %d): ", #c, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct HostAlloc {
    static long long live_bytes, live_blocks, peak_bytes, allocs, frees;
    static long long fail_at; // the allocation with this running number fails (-1: none)
    static int alloc(void **p, size_t bytes) {
        if (allocs++ == fail_at) {
            *p = nullptr;
            return 2; // ("out of memory")
        }
        *p = malloc(bytes ? bytes : 1);
        memset(*p, 0xab, bytes);
        live_bytes += (long long)bytes;
        live_blocks++;
        if (live_bytes > peak_bytes) peak_bytes = live_bytes;
        return 0;
    }
    static int free(void *p, size_t bytes) {
        live_bytes -= (long long)bytes;
        live_blocks--;
        frees++;
        ::free(p);
        return 0;
    }
    static void reset_counters() {
        peak_bytes = live_bytes;
        allocs = frees = 0;
        fail_at = -1;
    }
};
long long HostAlloc::live_bytes = 0, HostAlloc::live_blocks = 0, HostAlloc::peak_bytes = 0, HostAlloc::allocs = 0, HostAlloc::frees = 0;
long long HostAlloc::fail_at = -1;

template <class T> using HBuf = dppr::Buf<T, HostAlloc>;

static_assert(!std::is_copy_constructible<HBuf<int>>::value && !std::is_copy_assignable<HBuf<int>>::value, "an owner is never copied");
static_assert(std::is_nothrow_move_constructible<HBuf<int>>::value, "a vector of owners grows by moves");
static_assert(sizeof(HBuf<double>) == sizeof(double *) + sizeof(size_t), "pointer + count: a swap stays a few words");

// the shape of Slot / Group: several buffers, a pointer INTO one of them, plain fields
struct Owner {
    int tag = 0;
    HBuf<double> p, r;
    HBuf<unsigned> act[2];
    HBuf<int> cnt;
    int *log = nullptr; // cnt + 4
    std::vector<int> trace;
};
static_assert(!std::is_copy_constructible<Owner>::value && std::is_nothrow_move_constructible<Owner>::value, "a struct of owners moves only");

// what dppr_add_source does: fill a local owner step by step, give up at the first failure
static int build_owner(Owner &o, size_t n, int tag) {
    o.tag = tag;
    if (int rc = o.p.alloc(n)) return rc;
    if (int rc = o.r.alloc(n)) return rc;
    if (int rc = o.act[0].alloc(n / 32 + 1)) return rc;
    if (int rc = o.act[1].alloc(n / 32 + 1)) return rc;
    if (int rc = o.cnt.alloc(16)) return rc;
    o.log = o.cnt + 4;
    o.p[0] = tag;
    o.cnt[4] = tag;
    return 0;
}

static void take_ptr(const double *) {}

static void basics() {
    HostAlloc::reset_counters();
    {
        HBuf<double> a;
        CHECK(a.get() == nullptr && a.capacity() == 0 && !a, "default state is empty");
        CHECK(a.alloc(100) == 0 && a.capacity() == 100 && a, "alloc");
        CHECK(HostAlloc::live_bytes == 800 && HostAlloc::live_blocks == 1, "%lld bytes", HostAlloc::live_bytes);
        double *raw = a; // implicit conversion, pointer arithmetic, indexing
        take_ptr(a);
        CHECK(raw == a.get() && a + 3 == raw + 3 && &a[5] == raw + 5, "conversion to T *");
        a[7] = 1.5;
        HBuf<double> b(std::move(a));
        CHECK(!a && a.capacity() == 0 && b.get() == raw && b.capacity() == 100 && b[7] == 1.5, "move construction transfers");
        CHECK(HostAlloc::allocs == 1 && HostAlloc::frees == 0, "a move allocates and frees nothing");
        HBuf<double> c;
        c = std::move(b);
        CHECK(!b && c.get() == raw && c.capacity() == 100, "move assignment onto an empty buffer transfers");
        HBuf<double> d;
        CHECK(d.alloc(10) == 0, "alloc");
        double *rawd = d;
        std::swap(c, d); // (what the loops do with x / x2 and the activity bitmaps)
        CHECK(c.get() == rawd && c.capacity() == 10 && d.get() == raw && d.capacity() == 100, "std::swap exchanges");
        swap(c, d);
        c.swap(d);
        CHECK(c.get() == rawd && d.get() == raw, "swap twice is the identity");
        CHECK(HostAlloc::allocs == 2 && HostAlloc::frees == 0 && HostAlloc::live_blocks == 2, "swaps allocate and free nothing");
        d.reset();
        CHECK(!d && d.capacity() == 0 && HostAlloc::live_bytes == 80 && HostAlloc::frees == 1, "reset releases");
        d.reset();
        CHECK(HostAlloc::frees == 1, "reset of an empty buffer does nothing");
    }
    CHECK(HostAlloc::live_bytes == 0 && HostAlloc::live_blocks == 0, "destruction releases: %lld bytes live", HostAlloc::live_bytes);
}

static void regrow_and_failure() {
    HostAlloc::reset_counters();
    {
        HBuf<int> a;
        CHECK(a.regrow(1000) == 0 && a.capacity() == 1000, "regrow of an empty buffer allocates");
        HostAlloc::reset_counters();
        CHECK(a.regrow(3000) == 0 && a.capacity() == 3000, "regrow");
        CHECK(HostAlloc::peak_bytes == 12000 && HostAlloc::live_bytes == 12000 && HostAlloc::live_blocks == 1,
              "regrow releases BEFORE it allocates: peak %lld", HostAlloc::peak_bytes);
        HostAlloc::reset_counters();
        HostAlloc::fail_at = 0;
        CHECK(a.regrow(5000) == 2, "the allocator's status is returned");
        CHECK(!a && a.capacity() == 0 && HostAlloc::live_bytes == 0 && HostAlloc::live_blocks == 0, "a failed regrow leaves an empty buffer");
        HostAlloc::fail_at = 1;
        HBuf<int> b;
        CHECK(b.alloc(5) == 2 && !b && b.capacity() == 0, "a failed alloc leaves an empty buffer");
        CHECK(b.alloc(5) == 0 && b.capacity() == 5, "... that can be allocated again");
        CHECK(a.regrow(0) == 0, "zero elements");
    }
    CHECK(HostAlloc::live_bytes == 0 && HostAlloc::live_blocks == 0, "%lld bytes live", HostAlloc::live_bytes);
}

static void owners() {
    // built up to a failing allocation and dropped: nothing stays behind, whichever allocation fails
    for (int k = 0; k <= 5; ++k) {
        HostAlloc::reset_counters();
        HostAlloc::fail_at = k < 5 ? k : -1;
        {
            Owner o;
            const int rc = build_owner(o, 1000, 7);
            CHECK((rc != 0) == (k < 5), "allocation %d fails", k);
            CHECK(HostAlloc::live_blocks == (k < 5 ? k : 5), "%lld blocks live while the local exists", HostAlloc::live_blocks);
        }
        CHECK(HostAlloc::live_bytes == 0 && HostAlloc::live_blocks == 0, "failure at %d leaks %lld bytes", k, HostAlloc::live_bytes);
    }
    // a vector of owners grown past its capacity: every buffer (and every pointer into one) intact, nothing allocated or freed by the moves
    HostAlloc::reset_counters();
    {
        std::vector<Owner> v;
        std::vector<const double *> where;
        for (int i = 0; i < 100; ++i) {
            Owner o;
            CHECK(build_owner(o, 64 + (size_t)i, i) == 0, "build");
            where.push_back(o.p.get());
            v.push_back(std::move(o));
            CHECK(!o.p && !o.cnt && o.p.capacity() == 0, "the moved-from local owns nothing");
        }
        CHECK(HostAlloc::allocs == 500 && HostAlloc::frees == 0 && HostAlloc::live_blocks == 500, "moves: %lld allocs %lld frees", HostAlloc::allocs, HostAlloc::frees);
        for (int i = 0; i < 100; ++i) {
            const Owner &o = v[(size_t)i];
            CHECK(o.tag == i && o.p.get() == where[(size_t)i] && o.p[0] == i && o.p.capacity() == 64 + (size_t)i, "owner %d moved intact", i);
            CHECK(o.log == o.cnt + 4 && *o.log == i, "the pointer into cnt of owner %d still points into it", i);
        }
        std::swap(v[10], v.back()); // (an owner that holds memory is never assigned to -- no erase in the middle --; a swap is moves)
        v.pop_back();
        CHECK(HostAlloc::live_blocks == 495 && HostAlloc::frees == 5 && v[10].tag == 99 && v[10].p[0] == 99, "swap and drop the last");
    }
    CHECK(HostAlloc::live_bytes == 0 && HostAlloc::live_blocks == 0, "%lld bytes live", HostAlloc::live_bytes);
}

// random sequences of every operation against a model of who owns how many elements
static void random_ops(std::mt19937 &rng, int steps) {
    HostAlloc::reset_counters();
    {
        std::vector<HBuf<long long>> pool(8);
        std::vector<size_t> model(8, 0);
        std::vector<Owner> owners;
        for (int s = 0; s < steps && fails == 0; ++s) {
            const size_t i = rng() % 8, j = rng() % 8, n = rng() % 500;
            HostAlloc::fail_at = rng() % 7 == 0 ? HostAlloc::allocs : -1; // every seventh step: the next allocation fails
            const bool will_fail = HostAlloc::fail_at >= 0;
            switch (rng() % 8) {
            case 0:
                if (!pool[i]) {
                    CHECK((pool[i].alloc(n) != 0) == will_fail, "alloc");
                    model[i] = will_fail ? 0 : n;
                }
                break;
            case 1:
                CHECK((pool[i].regrow(n) != 0) == will_fail, "regrow");
                model[i] = will_fail ? 0 : n;
                break;
            case 2:
                pool[i].reset();
                model[i] = 0;
                break;
            case 3:
                std::swap(pool[i], pool[j]);
                std::swap(model[i], model[j]);
                break;
            case 4:
                if (i != j && !pool[i]) { // (an owner that holds memory is never assigned to: asserted by the type)
                    pool[i] = std::move(pool[j]);
                    model[i] = model[j];
                    model[j] = 0;
                }
                break;
            case 5: {
                HBuf<long long> t(std::move(pool[i]));
                CHECK(!pool[i] && t.capacity() == model[i], "move construction");
                pool[i].swap(t);
                break;
            }
            case 6: {
                Owner o;
                if (build_owner(o, 32 + n, s) == 0) owners.push_back(std::move(o)); // (a failed one is dropped half built)
                break;
            }
            default:
                if (!owners.empty()) {
                    std::swap(owners[rng() % owners.size()], owners.back());
                    owners.pop_back();
                }
            }
            long long want = 0;
            for (size_t k = 0; k < 8; ++k) {
                CHECK(pool[k].capacity() == model[k] && (pool[k].get() != nullptr || model[k] == 0), "buffer %zu holds %zu, model says %zu", k, pool[k].capacity(), model[k]);
                if (model[k]) pool[k][model[k] - 1] = (long long)s; // (ASan: the last element is ours)
                want += (long long)(model[k] * sizeof(long long));
            }
            for (const Owner &o : owners) want += (long long)(sizeof(double) * 2 * o.p.capacity() + sizeof(unsigned) * 2 * o.act[0].capacity() + sizeof(int) * 16);
            CHECK(HostAlloc::live_bytes == want, "step %d: %lld bytes live, the model says %lld", s, HostAlloc::live_bytes, want);
        }
        HostAlloc::fail_at = -1;
    }
    CHECK(HostAlloc::live_bytes == 0 && HostAlloc::live_blocks == 0, "random sequence ends with %lld bytes in %lld blocks", HostAlloc::live_bytes,
          HostAlloc::live_blocks);
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    const int cases = argc > 2 ? atoi(argv[2]) : 20;
    std::mt19937 rng(seed);
    basics();
    regrow_and_failure();
    owners();
    for (int c = 0; c < cases && fails == 0; ++c) random_ops(rng, 2000);
    printf("devbuf_test seed %u: %d cases, %d failures\n", seed, cases, fails);
    return fails ? 1 : 0;
}
