// ms_order.h — the cross-stream ordering protocol of a context, as one class.
// Host only, no HIP: the policy that names the runtime calls is in ms_ctx.h,
// and tests/cpp/test_order.cpp runs this header under ASan over a model of
// streams and events that tracks happens-before sets.
//
// Ordering. Every piece of work that reads or writes the node table or the
// context's scratch is totally ordered through the context stream. The
// invariant (the one the model test checks): every ordered piece of work
// happens after every ordered piece of work enqueued before it, whichever
// streams the two ran on.
//
// A call on a caller stream first waits for the context stream (enter), and
// its work is then chained back into the context stream (leave), so later
// deltas, binds, read-backs and calls on any other stream wait for it. A call
// on the context stream itself needs neither. seq() counts enqueues on the
// context stream that a caller stream has not necessarily seen; a caller
// stream ordered after it at seq() needs no new cross-stream wait (each costs
// ~6-10 us of idle device time even when already signalled,
// tools/ubench/xstream). The fence count does the same for the times the
// context stream was made to wait for the communicator's in-flight sweeps
// (table readers on its internal streams, comm_fence_reads): a stream ordered
// before the last fence must wait again.
//
// A policy P gives `stream` (comparable handles), `event` (default
// constructed empty; created lazily by record), `bool record(event &, stream)`
// and `bool wait(stream, event &)`, both false on failure.
#pragma once

#include <cstdint>
#include <utility>

namespace msgpu {

template <class P>
class StreamOrder {
  public:
    using stream = typename P::stream;
    using event = typename P::event;
    explicit StreamOrder(P p = P()) : p_(std::move(p)) {}

    // The context stream (once, when it exists).
    void attach(stream ctx) { ctx_ = ctx; }

    // Enqueues on the context stream a caller stream has not necessarily seen:
    // compared by the communicator's sweep streams (ms_comm.cpp prepare_locked).
    uint64_t seq() const { return ctx_seq_; }
    // Work was enqueued on the context stream outside enter / leave (deltas, a
    // bind, a host-array cycle): a caller stream ordered earlier waits again.
    void wrote_ctx() { ++ctx_seq_; }
    // The context stream was made to wait for the communicator's table readers.
    void fenced() { ++fence_seq_; }

    // Before a call's first launch on s: s waits for everything already on the
    // context stream, unless s was ordered after it with nothing new since.
    // fenced: comm_fence_reads inserted waits into the context stream for this call.
    bool enter(stream s, bool was_fenced) {
        if (was_fenced) fenced();
        if (s == ctx_) return true;
        if (s == ordered_stream_ && ordered_seq_ == ctx_seq_ && ordered_fence_ == fence_seq_)
            return true;  // nothing new on the context stream
        if (!p_.record(ev_order_, ctx_) || !p_.wait(s, ev_order_)) return false;
        ordered_stream_ = s;
        ordered_seq_ = ctx_seq_;
        ordered_fence_ = fence_seq_;
        return true;
    }

    // After the last launch of a call that entered with s. A caller stream:
    // the context stream waits for it; s itself needs no new wait afterwards
    // (it stays the ordered stream), any other stream does. The context
    // stream: the call enqueued there, so the sequence advances and a caller
    // stream ordered earlier waits again.
    // recorded: back_event() was already recorded on s after the call's last
    // launch (by that launch's own dispatch).
    bool leave(stream s, bool recorded = false) {
        if (s == ctx_) {
            wrote_ctx();
            return true;
        }
        if (!recorded && !p_.record(ev_back_, s)) return false;
        return p_.wait(ctx_, ev_back_);
    }

    // The chain-back event, for a dispatch that records it itself (leave's `recorded`).
    event &back_event() { return ev_back_; }

  private:
    P p_;
    stream ctx_{};
    uint64_t ctx_seq_ = 0;
    uint64_t fence_seq_ = 0, ordered_fence_ = 0;
    stream ordered_stream_{};  // (not owned: a caller's)
    uint64_t ordered_seq_ = 0;
    event ev_order_, ev_back_;
};

}  // namespace msgpu
