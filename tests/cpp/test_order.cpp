// The cross-stream ordering protocol of a context
// (mini-kube-scheduler_amd/csrc/ms_order.h) over the model of streams and
// events in order_model.h (happens-before sets per stream). The
// driver uses the class the way the library's call guard does (enter, one
// piece of work on the stream, leave), with flushes and binds on the context
// stream between calls and fences reported or not, and checks
//   1. the invariant: every piece of work happens after every ordered piece
//      of work enqueued before it;
//   2. no extra waits: the class records and waits exactly as often as the
//      rule it replaced (ParentOrder below, transcribed from the functions
//      order_after_ctx_stream / chain_back of the parent revision), except in
//      sequences where that rule broke the invariant.
// Built under ASan/UBSan by tests/test_host_cpp.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "ms_order.h"
#include "order_model.h"

using namespace msgpu;

namespace {

constexpr int kCtx = 0, kA = 1, kB = 2, kStreams = 3;

template <int N>
using World = order_model::World<N, kStreams>;
template <int N>
using ModelPolicy = order_model::ModelPolicy<N, kStreams>;
template <int N>
World<N> *&world() {
    return order_model::world<N, kStreams>();
}

// The rule before ms_order.h, from the parent revision's order_after_ctx_stream
// (enter) and chain_back (leave): a call on the context stream moves no counter.
template <class P>
class ParentOrder {
  public:
    using stream = typename P::stream;
    using event = typename P::event;
    explicit ParentOrder(P p = P()) : p_(p) {}
    void attach(stream ctx) { ctx_ = ctx; }
    void wrote_ctx() { ++ctx_seq; }
    void fenced() { ++fence_seq; }
    bool enter(stream s, bool was_fenced) {
        if (was_fenced) ++fence_seq;
        if (s == ctx_) return true;
        if (s == ordered_stream && ordered_seq == ctx_seq && ordered_fence == fence_seq) return true;
        if (!p_.record(ev_order, ctx_) || !p_.wait(s, ev_order)) return false;
        ordered_stream = s;
        ordered_seq = ctx_seq;
        ordered_fence = fence_seq;
        return true;
    }
    bool leave(stream s, bool recorded = false) {
        if (s == ctx_) return true;
        if (!recorded && !p_.record(ev_back, s)) return false;
        if (!p_.wait(ctx_, ev_back)) return false;
        if (ordered_stream != s) {
            ++ctx_seq;
            ordered_stream = s;
            ordered_seq = ctx_seq;
            ordered_fence = fence_seq;
        }
        return true;
    }
    event &back_event() { return ev_back; }

  private:
    P p_;
    stream ctx_{};
    uint64_t ctx_seq = 0, fence_seq = 0, ordered_fence = 0;
    stream ordered_stream = -1;  // (the library's null: no caller stream)
    uint64_t ordered_seq = 0;
    event ev_order, ev_back;
};

// One step of a sequence: a device call on `stream`, with deltas drained
// before it or not (flush_locked: work on the context stream, wrote_ctx), a
// fence reported to enter or not, and the chain-back event recorded by the
// call's own dispatch or by leave. bind: no call, a single bind instead (the
// fence counted by fenced(), work on the context stream, wrote_ctx).
struct Step {
    int stream;
    bool flush, fence, recorded, bind;
};

long failed = 0;
void check(bool ok, const char *what, long k = -1) {
    if (ok) return;
    if (failed++ < 20) std::printf("FAIL %s (k = %ld)\n", what, k);
}

// A rule with the world it acts on.
template <template <class> class Rule, int N>
struct Sim {
    World<N> w;
    Rule<ModelPolicy<N>> r;
    Sim() { r.attach(kCtx); }
    bool step(const Step &st) {
        world<N>() = &w;
        if (st.bind) {
            if (st.fence) {
                w.fence();
                r.fenced();
            }
            w.work(kCtx);
            r.wrote_ctx();
            return true;
        }
        if (st.flush) {
            w.work(kCtx);
            r.wrote_ctx();
        }
        if (st.fence) w.fence();
        if (!r.enter(st.stream, st.fence)) return false;
        w.work(st.stream);
        const bool recorded = st.recorded && st.stream != kCtx;  // (the guard hands out no event on the context stream)
        if (recorded && !ModelPolicy<N>::record(r.back_event(), st.stream)) return false;
        return r.leave(st.stream, recorded);
    }
};

template <int N>
using NewSim = Sim<StreamOrder, N>;
template <int N>
using OldSim = Sim<ParentOrder, N>;

Step call(int stream, bool flush = false, bool fence = false, bool recorded = false) {
    return Step{stream, flush, fence, recorded, false};
}

// Both rules over one sequence; the counts must agree while the parent's rule
// still holds the invariant.
template <int N>
struct Pair {
    NewSim<N> a;
    OldSim<N> b;
    void step(const Step &st, long k = -1) {
        check(a.step(st), "the class reported a failure the model never injected", k);
        check(!a.w.violated, "invariant: a piece of work does not follow an earlier ordered one", k);
        check(!a.w.bad_wait, "wait for an event never recorded", k);
        if (b.w.violated) return;  // (nothing left to compare with in this sequence)
        check(b.step(st), "the parent rule reported a failure the model never injected", k);
        check(!b.w.bad_wait, "parent rule: wait for an event never recorded", k);
        if (!b.w.violated)
            check(a.w.waits == b.w.waits && a.w.records == b.w.records && a.w.events_made == b.w.events_made,
                  "waits / records differ from the parent rule where that rule held the invariant", k);
    }
};

long nodes = 0, parent_violations = 0;

// Every sequence of at most `left` more steps after the state in p.
void search(const Pair<1> &p, int left) {
    if (left == 0) return;
    for (int s = 0; s < kStreams; ++s)
        for (int flush = 0; flush < 2; ++flush)
            for (int fence = 0; fence < 2; ++fence)
                for (int rec = 0; rec < (s == kCtx ? 1 : 2); ++rec) {  // (recorded means nothing on the context stream)
                    Pair<1> q = p;
                    q.step(call(s, flush, fence, rec), nodes);
                    ++nodes;
                    if (q.b.w.violated && !p.b.w.violated) ++parent_violations;
                    search(q, left - 1);
                }
}

void named_cases() {
    {  // the sequence that motivated the class: caller stream, context stream, the caller stream again
        Pair<1> p;
        p.step(call(kA));
        p.step(call(kCtx));
        check(!p.b.w.violated, "parent rule: the first two calls are ordered");
        check(p.a.w.waits == 2 && p.b.w.waits == 2, "two calls: one wait in, one wait back");
        p.step(call(kA));
        check(!p.a.w.violated, "caller / context / caller: the third call follows the second");
        check(p.b.w.violated, "caller / context / caller: the parent rule is expected to miss the wait (the model must see it)");
        check(p.a.w.waits == 4 && p.b.w.waits == 3, "caller / context / caller: one wait more than the parent rule");
    }
    {  // the same with the fused dispatch recording the chain-back event itself
        Pair<1> p;
        p.step(call(kA, false, false, true));
        p.step(call(kCtx));
        p.step(call(kA, false, false, true));
        check(!p.a.w.violated && p.b.w.violated, "caller / context / caller, recorded by the dispatch");
    }
    {  // back-to-back calls on one caller stream: one wait in, then only the chain-backs
        Pair<1> p;
        for (int i = 0; i < 4; ++i) p.step(call(kA));
        check(!p.b.w.violated, "back-to-back: parent rule holds");
        check(p.b.w.records == 5 && p.b.w.waits == 5 && p.b.w.events_made == 2, "back-to-back: parent counts");
        check(p.a.w.records == 5 && p.a.w.waits == 5 && p.a.w.events_made == 2, "back-to-back: 5 records, 5 waits");
    }
    {  // context-stream-only sequences: no event, no wait, whatever else happens there
        Pair<1> p;
        for (int i = 0; i < 6; ++i) p.step(call(kCtx, i & 1, i & 2));
        p.step(Step{kCtx, false, true, false, true});
        check(!p.b.w.violated, "context stream only: parent rule holds");
        check(p.b.w.records == 0 && p.b.w.waits == 0 && p.b.w.events_made == 0, "context stream only: parent counts");
        check(p.a.w.records == 0 && p.a.w.waits == 0 && p.a.w.events_made == 0, "context stream only: no event, no wait");
    }
    {  // one caller stream, deltas drained before every call: every call waits in and chains back
        Pair<1> p;
        for (int i = 0; i < 4; ++i) p.step(call(kA, true));
        check(!p.b.w.violated, "flush before every call: parent rule holds");
        check(p.b.w.records == 8 && p.b.w.waits == 8, "flush before every call: parent counts");
        check(p.a.w.records == 8 && p.a.w.waits == 8, "flush before every call: 8 records, 8 waits");
    }
    {  // two caller streams alternate: each call waits for the other's chained-back work
        Pair<1> p;
        for (int i = 0; i < 4; ++i) p.step(call(i & 1 ? kB : kA));
        check(!p.a.w.violated && !p.b.w.violated, "alternating caller streams");
        check(p.a.w.waits == 8 && p.b.w.waits == 8, "alternating caller streams: a wait in and one back per call");
    }
    {  // a fence alone makes the ordered stream wait again
        Pair<1> p;
        p.step(call(kA));
        p.step(call(kA, false, true));
        check(!p.a.w.violated && !p.b.w.violated, "fence reported to enter");
        check(p.a.w.waits == 4, "fence: the ordered stream waits again");
        p.step(Step{kCtx, false, true, false, true});  // a bind that fenced
        p.step(call(kA));
        check(!p.a.w.violated && p.a.w.waits == 6, "fence counted by a bind");
    }
    {  // a failed record or wait is reported and leaves the stream unordered: the next call waits
        NewSim<1> a;
        check(a.step(call(kCtx)), "context call");
        a.w.fail_in = 2;  // enter's wait
        check(!a.step(call(kA)), "enter reports the failed wait");
        a.w.fail_in = 0;
        const long before = a.w.waits;
        check(a.step(call(kA)) && a.w.waits == before + 2 && !a.w.violated, "after a failed enter the stream waits");
        a.w.fail_in = 1;  // leave's record
        check(!a.step(call(kA)), "leave reports the failed record");
    }
}

void random_sequences() {
    std::mt19937 rng(20261020u);
    for (int seq = 0; seq < 4000; ++seq) {
        Pair<4> p;  // (50 steps of at most 3 ids each)
        // per sequence its own mix, so that long runs on one stream occur as well as churn
        const unsigned p_ctx = rng() % 4, p_flush = rng() % 4, p_fence = rng() % 6, p_bind = rng() % 8;
        for (int i = 0; i < 50; ++i) {
            Step st{};
            st.bind = p_bind && rng() % 8 < p_bind / 2;
            st.stream = rng() % 4 < p_ctx ? kCtx : (rng() & 1 ? kA : kB);
            st.flush = rng() % 4 < p_flush;
            st.fence = rng() % 8 < p_fence;
            st.recorded = rng() & 1;
            p.step(st, seq);
        }
        if (p.b.w.violated) ++parent_violations;
    }
}

}  // namespace

int main() {
    named_cases();
    search(Pair<1>(), 6);
    std::printf("sequences up to length 6 checked: %ld (the parent rule first breaks the invariant in %ld)\n", nodes,
                parent_violations);
    check(nodes == 20 + 400 + 8000 + 160000 + 3200000 + 64000000, "search size");
    check(parent_violations > 0, "the search meets sequences where the parent rule fails");
    parent_violations = 0;
    random_sequences();
    std::printf("random sequences of length 50 checked: 4000 (the parent rule breaks the invariant in %ld)\n",
                parent_violations);
    std::printf("%ld failed\n", failed);
    return failed ? 1 : 0;
}
