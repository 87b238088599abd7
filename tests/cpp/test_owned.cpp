// The owner type behind every device buffer, pinned buffer, event and stream of
// the library (mini-kube-scheduler_amd/csrc/ms_owned.h), with a counting
// malloc/free policy that can be told to fail its k-th allocation. Built under
// ASan/UBSan with leak detection by tests/test_host_cpp.py: a block released
// twice, used after release or never released stops the run, whatever the
// counters below say.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "ms_owned.h"

using namespace msgpu;

namespace {

long live = 0, acquired = 0, released = 0;
long fail_at = 0;  // the k-th acquire from now fails (1 = the next one); 0 = none

struct Counting {
    using handle = char *;
    static char *acquire(size_t n) {
        if (fail_at && --fail_at == 0) return nullptr;
        char *p = static_cast<char *>(std::malloc(n ? n : 1));
        if (p) {
            std::memset(p, 0xA5, n ? n : 1);
            ++live;
            ++acquired;
        }
        return p;
    }
    static void release(char *p) {
        std::free(p);
        --live;
        ++released;
    }
};
using Buf = Owned<Counting>;

// A handle with no size: acquired lazily, like the library's events.
struct CountingEvent {
    using handle = int *;
    static int *acquire() {
        ++live;
        return new int(7);
    }
    static void release(int *p) {
        delete p;
        --live;
    }
};

long failed = 0;
void check(bool ok, const char *what, long k = -1) {
    if (ok) return;
    if (failed++ < 20) std::printf("FAIL %s (k = %ld, live = %ld)\n", what, k, live);
}

// Shaped like ensure_tiles: a capacity and 11 members grown together; the
// capacity is zero whenever the group is not whole.
struct Group {
    static constexpr int kMembers = 11;
    Buf m[kMembers];
    size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        cap = 0;
        for (int i = 0; i < kMembers; ++i)
            if (!m[i].alloc(n * (size_t)(i + 1))) return false;
        cap = n;
        return true;
    }
    bool whole() const {
        for (const Buf &b : m)
            if (!b) return false;
        return true;
    }
};

}  // namespace

int main() {
    // the destructor releases once; an owner that never held anything releases nothing
    {
        Buf a, none;
        check(!a && a.get() == nullptr, "a new owner holds nothing");
        check(a.alloc(64) && a && live == 1, "alloc");
        a.get()[63] = 1;
        char *raw = a;  // the implicit conversion call sites use
        check(raw == a.get(), "implicit conversion");
    }
    check(live == 0 && acquired == 1 && released == 1, "destructor releases once");

    // move construction transfers; the source holds nothing and releases nothing
    {
        Buf a;
        check(a.alloc(32), "alloc");
        char *p = a.get();
        Buf b(std::move(a));
        check(!a && b.get() == p && live == 1, "move construction");
    }
    check(live == 0 && released == 2, "moved-from and moved-to release once between them");

    // move assignment releases the target's old block and transfers the source's
    {
        Buf a, b;
        check(a.alloc(16) && b.alloc(48) && live == 2, "two blocks");
        char *p = a.get();
        b = std::move(a);
        check(live == 1 && !a && b.get() == p, "move assignment releases the old block");
        b = std::move(b);  // (self-assignment keeps the block)
        check(live == 1 && b.get() == p, "self move assignment");
        Buf empty;
        b = std::move(empty);
        check(live == 0 && !b, "assignment from an empty owner releases");
    }
    check(live == 0, "after move assignment");

    // alloc on a live owner releases first; a failed alloc leaves nothing; reset twice is harmless
    {
        Buf a;
        check(a.alloc(8) && a.alloc(24) && live == 1 && released == acquired - 1, "alloc on a live owner releases first");
        fail_at = 1;
        check(!a.alloc(100) && !a && a.get() == nullptr && live == 0, "a failed alloc leaves null");
        check(a.alloc(100) && live == 1, "alloc after a failure");
        a.reset();
        a.reset();
        check(!a && live == 0, "reset twice");
    }
    check(live == 0 && acquired == released, "after alloc / reset");

    // ensure acquires once
    {
        Owned<CountingEvent> e;
        check(e.ensure() && live == 1, "ensure creates");
        int *p = e.get();
        check(e.ensure() && e.get() == p && live == 1 && *p == 7, "ensure keeps what is held");
    }
    check(live == 0, "after ensure");

    // group growth: failure at each position k of the 11-member chain, on a fresh group
    // and on one that already holds smaller blocks; then the retry, then the destructor
    for (int grown = 0; grown < 2; ++grown)
        for (long k = 1; k <= Group::kMembers; ++k) {
            {
                Group g;
                if (grown) check(g.ensure(10) && g.whole() && g.cap == 10 && live == Group::kMembers, "first growth", k);
                fail_at = k;
                check(!g.ensure(100), "growth fails at k", k);
                check(g.cap == 0, "capacity is zero while the group is not whole", k);
                check(!g.m[k - 1], "the member that failed holds nothing", k);
                check(g.ensure(100) && g.whole() && g.cap == 100, "the retry succeeds", k);
                check(live == Group::kMembers, "one block per member after the retry", k);
                g.m[Group::kMembers - 1].get()[100 * Group::kMembers - 1] = 1;  // (the last byte is ours)
                check(g.ensure(50) && g.cap == 100, "no growth below the capacity", k);
            }
            check(live == 0, "live count after the group's destructor", k);
            {
                Group g;  // destroyed while not whole
                if (grown) check(g.ensure(10), "first growth", k);
                fail_at = k;
                check(!g.ensure(100), "growth fails at k", k);
            }
            check(live == 0, "live count after a failed group's destructor", k);
        }
    check(fail_at == 0 && acquired == released, "every block released once");
    std::printf("acquired %ld released %ld\n", acquired, released);
    std::printf("%ld failed\n", failed);
    return failed ? 1 : 0;
}
