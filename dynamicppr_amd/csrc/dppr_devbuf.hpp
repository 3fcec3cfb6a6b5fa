// dppr_devbuf.hpp -- the one owner type of the engine's device and pinned-host memory: Buf<T, Alloc> holds one allocation of
// `capacity()` elements and releases it when it goes out of scope. Pure host code without HIP includes (the engine supplies the two
// allocator policies, dppr_host_state.hpp; tests/native/devbuf_test.cpp drives the type on the CPU with a counting host allocator).
//   Alloc::alloc(void **p, size_t bytes) -> int status (0 = success), Alloc::free(void *p, size_t bytes) -> int status
//   (free is told the size so that a policy can keep a count of live bytes without a table of its own)
// A Buf moves, it is never copied; a move or a swap exchanges pointers and allocates / frees nothing. It converts to T *, so kernel
// launches, copies and pointer arithmetic read as with a raw pointer; a pointer INTO a buffer (Slot::log, Epoch::bcut) stays raw.
// Only regrow() and reset() -- and the destructor -- free: an owner is never the target of an assignment while it holds memory
// (asserted: a device free waits for the whole device, so a free hidden in an assignment inside a loop would be a silent stall).
#pragma once

#include <cassert>
#include <cstddef>
#include <utility>

namespace dppr {

template <class T, class Alloc>
class Buf {
    T *p_ = nullptr;
    size_t n_ = 0; // elements allocated

  public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), n_(o.n_) {
        o.p_ = nullptr;
        o.n_ = 0;
    }
    Buf &operator=(Buf &&o) noexcept {
        assert((!p_ || this == &o) && "move assignment onto a buffer that owns memory: reset() or regrow() it");
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~Buf() { reset(); }

    void swap(Buf &o) noexcept {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
    }
    friend void swap(Buf &a, Buf &b) noexcept { a.swap(b); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t capacity() const { return n_; } // elements (0: empty)

    // `count` elements into an EMPTY buffer; the allocator's status (a failure leaves the buffer empty)
    int alloc(size_t count) {
        assert(!p_ && "alloc() on a buffer that owns memory: regrow() it");
        void *q = nullptr;
        const int rc = Alloc::alloc(&q, sizeof(T) * count);
        if (rc != 0) return rc;
        p_ = static_cast<T *>(q);
        n_ = count;
        return 0;
    }
    // release, then allocate `count` elements (the old contents are gone either way)
    int regrow(size_t count) {
        reset();
        return alloc(count);
    }
    void reset() {
        if (p_) (void)Alloc::free(p_, sizeof(T) * n_);
        p_ = nullptr;
        n_ = 0;
    }
};

} // namespace dppr
