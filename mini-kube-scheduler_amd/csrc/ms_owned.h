// ms_owned.h — the one owner of a device buffer, pinned buffer, event or stream:
// a move-only handle that releases what it holds when it dies. Host only, no
// HIP: the policies that name the runtime calls are in ms_ctx.h, and
// tests/cpp/test_owned.cpp runs this header under ASan with a counting one.
// A policy P gives `handle` (a pointer type; handle{} is "nothing"),
// `static handle acquire(args...)` (handle{} on failure) and `static void release(handle)`.
#pragma once

#include <utility>

namespace msgpu {

template <class P>
class Owned {
  public:
    using handle = typename P::handle;
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, handle{})) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, handle{});
        }
        return *this;
    }
    ~Owned() { reset(); }

    handle get() const { return h_; }
    operator handle() const { return h_; }  // launch and copy call sites take the raw handle
    explicit operator bool() const { return h_ != handle{}; }
    void reset() {
        if (h_ != handle{}) P::release(std::exchange(h_, handle{}));
    }
    // Releases what is held, then acquires anew (buffers: the element count);
    // false, holding nothing, when the policy cannot.
    template <class... A>
    bool alloc(A... a) {
        reset();
        return (h_ = P::acquire(a...)) != handle{};
    }
    // Acquires only if nothing is held (the lazily created events and streams).
    template <class... A>
    bool ensure(A... a) {
        return h_ != handle{} || alloc(a...);
    }

  private:
    handle h_{};
};

}  // namespace msgpu
