// ms_shard_order.h — the cross-stream ordering of the node-sharded pipeline
// (ms_comm.cpp), as one class. Host only, no HIP and no RCCL: the policy that
// names the runtime calls is HipOrder in ms_ctx.h (the policy concept of
// ms_order.h), and tests/cpp/test_shard_order.cpp runs this header under ASan
// over the model of streams and events in tests/cpp/order_model.h.
//
// One batch crosses four streams: its sweep on X (the caller's stream, or one of
// two internal sweep streams), its collective on the collective stream, its
// decode on the decode stream, and the table's writers on the context stream.
// The invariant (the one the model test checks, per resource): every access
// happens after every earlier conflicting access to the same resource,
// whichever streams the two ran on. The resources are the node table, a
// batch's pods and results, and a slot's keys / flags, reduced keys / flags,
// census and gathered census (depth + 1 slots, used round robin).
//
// The rules, and why each wait suffices:
//  - begin: X follows the caller's stream (the pods); the context stream when
//    its sequence moved or another caller stream submits (table writes); and
//    the collective that read the slot's keys, submission k - depth - 1.
//    Collectives complete in issue order, so one wait covers all older ones:
//    X waits for submission k - L's and the next waits that one covers are
//    skipped. L = 2 (two steps old, normally done, and never the one the
//    previous sweep feeds). With coalesced submits L = 3: k is the first of a
//    pair (then k - 1 and k - 2 are the previous pair, whose collectives
//    follow the previous launch) or k - 3's wait is already on X. The held
//    submission is k - 1 at most, so k - L's collective has been recorded.
//    With depth + 1 <= L, or two sweep streams, X waits for the slot's own.
//  - a coalesced pair is one launch that records the second batch's sweep
//    event; that event covers both sweeps (covered_by_), for the collective
//    stream and for the fence.
//  - the collective of a slot follows its sweep and the drain that decoded the
//    slot's previous batch (it wrote what that decode read); one wait for the
//    newest drain covers every earlier one, so at most one wait per drain.
//  - a drain decodes the oldest k batches after the newest of their
//    collectives (issue order again) and stamps their slots with its number.
//  - the fence: every sweep in flight is the newest of its slot (a slot is
//    swept again only after the collective that read its previous sweep), so
//    a table writer waits for each used slot's sweep event.
//  - the TaintToleration two-pass form sweeps twice: the census (recorded; the
//    collective stream gathers after it), X after the all-gather, then the
//    picks, recorded on the same sweep event again, so the fence and the
//    reduce-scatter follow the picks.
//  - a slot's buffers are replaced only after its batch's decode was enqueued
//    (pending_through: with a submission held, the slot comes round while
//    that batch is still pending; the rule before this class missed it,
//    tests/cpp/test_shard_order.cpp named_cases).
// A submission whose sweep is held back for a partner (hold) has no sweep on
// the device yet: fence and drained_to refuse to run until it was swept, so
// ms_comm.cpp cannot forget to flush it. regrown refuses while the slot's
// batch is pending, so it cannot forget that drain either.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace msgpu {

template <class P>
class ShardOrder {
  public:
    using stream = typename P::stream;
    using event = typename P::event;
    static constexpr uint32_t kSlotsMax = 8;  // depth + 1 <= kSlotsMax

    // depth: batches in flight before the oldest are decoded; two_streams:
    // sweeps alternate over two internal streams instead of the caller's.
    ShardOrder(uint32_t depth, bool two_streams, P p = P())
        : p_(std::move(p)), depth_(std::min(depth, kSlotsMax - 1)), two_(two_streams) {}

    // ctx: the context stream; coll, dec: collective and decode streams;
    // sweep0 / sweep1: the internal sweep streams (two_streams only).
    void attach(stream ctx, stream coll, stream dec, stream sweep0 = stream(), stream sweep1 = stream()) {
        ctx_ = ctx, cs_ = coll, ds_ = dec, ss_[0] = sweep0, ss_[1] = sweep1;
    }

    bool two_streams() const { return two_; }
    // The slot of the next submission (its buffers are sized before begin).
    uint32_t next_slot() const { return (uint32_t)(submitted_ % (depth_ + 1)); }
    // How many of the oldest pending batches a drain must decode before the
    // slot's buffers may be replaced: 0 unless the batch that went through the
    // slot is still pending. (While a submission is held the next one's slot
    // comes round one step early: up to depth batches pending, the held one,
    // and the new one make depth + 2. Its keys were read, which is all the
    // sweep needs, but its decode still reads the reduced keys.)
    size_t pending_through(uint32_t slot) const {
        for (size_t i = 0; i < count_; ++i)
            if (pending_slot(i) == slot) return i + 1;
        return 0;
    }
    // The slot's buffers were replaced (its previous batch has been drained,
    // and the release of the old blocks waited for it): it starts over as
    // unused. False, and nothing changed, while that batch is pending.
    bool regrown(uint32_t slot) {
        if (pending_through(slot)) return false;
        used_[slot] = false;
        dec_gen_[slot] = 0;
        return true;
    }

    // Submission k, into next_slot(), on the caller's stream s: picks the sweep
    // stream X and orders it (see above). ctx_seq: the context's StreamOrder::seq().
    // pairs: sweeps may share a launch with the next submission's.
    bool begin(stream s, uint64_t ctx_seq, bool pairs, stream &X) {
        const uint64_t k = submitted_;
        const uint32_t si = next_slot(), xi = (uint32_t)(k & 1u);
        X = two_ ? ss_[xi] : s;
        if (X != s && (!p_.record(ev_in_, s) || !p_.wait(X, ev_in_))) return false;
        if (!ctx_known_ || ctx_seen_ != ctx_seq || ctx_seen_stream_ != s) {
            if (!p_.record(ev_ctx_, ctx_) || !p_.wait(X, ev_ctx_)) return false;
            if (two_ && !p_.wait(ss_[xi ^ 1u], ev_ctx_)) return false;
            ctx_known_ = true;
            ctx_seen_ = ctx_seq;
            ctx_seen_stream_ = s;
        }
        if (used_[si]) {
            const uint64_t prev = k - (depth_ + 1);
            const uint32_t L = pairs ? 3u : 2u;
            if (two_ || depth_ + 1 <= L) {
                if (!p_.wait(X, ev_comb_[si])) return false;
            } else if (!x_known_ || x_stream_ != X || x_comb_seen_ <= prev) {
                if (!p_.wait(X, ev_comb_[(k - L) % (depth_ + 1)])) return false;
                x_known_ = true;
                x_stream_ = X;
                x_comb_seen_ = k - L + 1;
            }
        }
        ++submitted_;
        return true;
    }

    // The submission just begun waits for a partner: nothing of it is on the
    // device until swept / swept_pair.
    void hold(uint32_t slot) { held_ = (int)slot; }
    bool held() const { return held_ >= 0; }

    // The slot's sweep event, for a dispatch that records it itself.
    event &sweep_event(uint32_t slot) { return ev_swept_[slot]; }

    // The slot's sweep is on X. recorded: its own dispatch recorded sweep_event(slot).
    bool swept(uint32_t slot, stream X, bool recorded) {
        if (!recorded && !p_.record(ev_swept_[slot], X)) return false;
        return note_swept(slot, slot);
    }
    // One launch swept the held batch (first) and this one (second) and
    // recorded sweep_event(second).
    bool swept_pair(uint32_t first, uint32_t second) { return note_swept(first, second) && note_swept(second, second); }

    // TaintToleration: the census is on X; the collective stream gathers after
    // it and after the drain whose final pass read the slot's gathered census.
    bool census_done(uint32_t slot, stream X) {
        return swept(slot, X, false) && coll_after_sweep(slot) && coll_after_drain(slot);
    }
    // The all-gather is on the collective stream: the picks on X follow it.
    bool gathered(uint32_t slot, stream X) { return p_.record(ev_ag_[slot], cs_) && p_.wait(X, ev_ag_[slot]); }

    // Before the slot's collective is issued: the collective stream follows the
    // sweep (unless it already does: a pair's second) and the drain that
    // decoded the slot's previous batch.
    bool before_collective(uint32_t slot) {
        if (!coll_after_sweep(slot) || !coll_after_drain(slot)) return false;
        used_[slot] = true;
        return true;
    }
    // The collective is on its stream: the batch is pending. n_drain: how many
    // of the oldest to decode now.
    bool after_collective(uint32_t slot, size_t &n_drain) {
        if (!p_.record(ev_comb_[slot], cs_)) return false;
        ring_[(head_ + count_++) % kSlotsMax] = slot;
        n_drain = count_ > depth_ ? std::min<size_t>(depth_, count_) : 0;
        return true;
    }

    size_t pending() const { return count_; }
    uint32_t pending_slot(size_t i) const { return ring_[(head_ + i) % kSlotsMax]; }

    // The decodes of the oldest k pending batches (k clamped; 0: nothing to do)
    // go on the decode stream between drain_begin and drain_end.
    bool drain_begin(size_t &k) {
        k = std::min(k, count_);
        return k == 0 || p_.wait(ds_, ev_comb_[pending_slot(k - 1)]);
    }
    bool drain_end(size_t k) {
        ++drains_;
        for (size_t i = 0; i < k; ++i) dec_gen_[pending_slot(i)] = drains_;
        if (!p_.record(ev_drained_, ds_)) return false;
        head_ = (uint32_t)((head_ + k) % kSlotsMax);
        count_ -= k;
        return true;
    }
    // After a drain of everything pending: s follows the decode stream.
    bool drained_to(stream s) { return !held() && count_ == 0 && p_.record(ev_ds_, ds_) && p_.wait(s, ev_ds_); }

    // A table writer on `writer` follows the sweeps in flight: 1 if waits were
    // inserted, 0 if no sweep ran since the last fence, < 0 on failure (or a
    // held submission: its sweep must be launched first).
    int fence(stream writer) {
        if (held()) return -1;
        if (!reads_outstanding_) return 0;
        for (uint32_t i = 0; i <= depth_; ++i)
            if (used_[i] && !p_.wait(writer, ev_swept_[covered_by_[i]])) return -1;
        reads_outstanding_ = false;
        return 1;
    }

  private:
    bool note_swept(uint32_t slot, uint32_t by) {
        covered_by_[slot] = by;
        if (held_ == (int)slot) held_ = -1;
        coll_swept_ = -1;
        reads_outstanding_ = true;
        return true;
    }
    bool coll_after_sweep(uint32_t slot) {
        const int by = (int)covered_by_[slot];
        if (coll_swept_ == by) return true;  // (a pair's second: the first one's wait)
        if (!p_.wait(cs_, ev_swept_[by])) return false;
        coll_swept_ = by;
        return true;
    }
    bool coll_after_drain(uint32_t slot) {
        if (!used_[slot] || dec_gen_[slot] <= cs_drain_seen_) return true;
        if (!p_.wait(cs_, ev_drained_)) return false;
        cs_drain_seen_ = drains_;
        return true;
    }

    P p_;
    uint32_t depth_;
    bool two_;
    stream ctx_{}, cs_{}, ds_{}, ss_[2] = {};
    event ev_swept_[kSlotsMax], ev_comb_[kSlotsMax], ev_ag_[kSlotsMax];
    event ev_in_, ev_ctx_;  // caller stream -> sweep stream, context stream -> sweep stream
    event ev_drained_;      // after the newest drain's decodes
    event ev_ds_;           // a drain to a stream
    // per slot: a collective went through it; the drain that decoded its last
    // batch; the slot whose sweep event was recorded after its sweep
    bool used_[kSlotsMax] = {};
    uint64_t dec_gen_[kSlotsMax] = {};
    uint32_t covered_by_[kSlotsMax] = {};
    uint32_t ring_[kSlotsMax] = {};  // pending slots, oldest first
    uint32_t head_ = 0;
    size_t count_ = 0;
    uint64_t submitted_ = 0;
    uint64_t drains_ = 0, cs_drain_seen_ = 0;  // drains enqueued / the newest the collective stream waited for
    int coll_swept_ = -1;                      // the sweep event the collective stream waited for last, still current
    int held_ = -1;                            // the slot of the held submission
    bool reads_outstanding_ = false;           // sweeps since the last fence
    bool ctx_known_ = false;
    uint64_t ctx_seen_ = 0;       // the context sequence the sweep streams were last ordered after
    stream ctx_seen_stream_{};    // (and the caller's stream then)
    bool x_known_ = false;
    uint64_t x_comb_seen_ = 0;    // x_stream_ waited for the collectives of submissions < this
    stream x_stream_{};
};

}  // namespace msgpu
