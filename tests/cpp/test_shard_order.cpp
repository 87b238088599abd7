// The ordering of the node-sharded pipeline
// (mini-kube-scheduler_amd/csrc/ms_shard_order.h) over the model of streams and
// events in order_model.h. The driver below uses the class the way ms_comm.cpp
// does (submit_locked, flush_stash, drain_to, comm_fence_reads, slot_ensure),
// with an access to a modelled resource wherever that file launches a kernel
// or a collective, and checks
//   1. the invariant, per resource: every access happens after every earlier
//      conflicting access to the same resource, whichever streams they ran on.
//      The node table (written on the context stream behind the fence, read by
//      every sweep, census and pick); a batch's pods (written on the caller's
//      stream before the submit, read by its sweep and its decode) and results
//      (written by its decode, read on the caller's stream after a drain to
//      it); a slot's keys / flags (sweep or picks -> collective), reduced keys
//      / flags (collective -> decode), census (census -> all-gather) and
//      gathered census (all-gather -> picks, final); d_tt (every
//      TaintToleration pass, exclusive);
//   2. no extra waits: the class records and waits exactly as often as the
//      rule it replaced (ParentShard below, transcribed from prepare_locked,
//      collective_locked, drain_locked, drain_to, comm_fence_reads and
//      tt2_sharded_sweep of the parent revision), in every sequence where
//      that rule holds the invariant; and it creates no more events (the
//      parent made all 28 at setup, the class makes one at its first record).
// Built under ASan/UBSan by tests/test_host_cpp.py.
#include <cstdint>
#include <cstdio>
#include <random>

#include "ms_shard_order.h"
#include "order_model.h"

using namespace msgpu;

namespace {

constexpr int kCtx = 0, kA = 1, kB = 2, kColl = 3, kDec = 4, kSweep0 = 5, kSweep1 = 6, kStreams = 7;
constexpr uint32_t kSlots = 8;

template <int N>
using World = order_model::World<N, kStreams>;
template <int N>
using Policy = order_model::ModelPolicy<N, kStreams>;
template <int N>
using Res = order_model::Resource<N>;

// The rule before ms_shard_order.h, with the state of the parent revision's
// CommState / ShardSlot under its names, cut at the same points as the class
// so that one driver runs both.
template <class P>
class ParentShard {
  public:
    using stream = typename P::stream;
    using event = typename P::event;
    ParentShard(uint32_t depth_, bool two) : two_streams(two), depth(depth_), group(depth_) {
        // (comm_setup created every event; a wait for one never recorded was legal and ordered nothing)
        for (uint32_t i = 0; i < kSlots; ++i) ev_swept[i].made = ev_comb[i].made = ev_ag[i].made = true;
        ev_in.made = ev_ctx.made = ev_drained.made = ev_ds.made = true;
    }
    void attach(stream ctx_, stream cs_, stream ds_, stream s0, stream s1) { ctx = ctx_, cs = cs_, ds = ds_, ss[0] = s0, ss[1] = s1; }
    uint32_t next_slot() const { return (uint32_t)(submitted % (depth + 1)); }
    size_t pending_through(uint32_t) const { return 0; }  // (slot_ensure never looked)
    bool regrown(uint32_t si) {  // slot_ensure
        used[si] = false;
        dec_gen[si] = 0;
        return true;
    }
    bool begin(stream s, uint64_t seq, bool coalescable, stream &X) {  // prepare_locked
        const uint32_t si = next_slot();
        const int xi = (int)(submitted & 1u);
        X = two_streams ? ss[xi] : s;
        if (X != s) {
            if (!P::record(ev_in, s)) return false;
            if (!P::wait(X, ev_in)) return false;
        }
        if (ctx_seen != seq || ctx_seen_stream != s) {
            if (!P::record(ev_ctx, ctx)) return false;
            if (!P::wait(X, ev_ctx)) return false;
            if (two_streams && !P::wait(ss[xi ^ 1], ev_ctx)) return false;
            ctx_seen = seq;
            ctx_seen_stream = s;
        }
        if (used[si]) {
            const uint64_t k = submitted, prev = k - (depth + 1);
            const uint32_t L = coalescable ? 3u : 2u;
            if (two_streams || depth + 1 <= L) {
                if (!P::wait(X, ev_comb[si])) return false;
            } else if (x_stream != X || x_comb_seen <= prev) {
                x_stream = X;
                if (!P::wait(X, ev_comb[(k - L) % (depth + 1)])) return false;
                x_comb_seen = k - L + 1;
            }
        }
        ++submitted;
        return true;
    }
    void hold(uint32_t) { stash_on = true; }
    bool held() const { return stash_on; }
    event &sweep_event(uint32_t si) { return ev_swept[si]; }
    bool swept(uint32_t si, stream X, bool recorded) {
        if (!recorded && !P::record(ev_swept[si], X)) return false;
        stash_on = false;  // (either the stash's own flush or no stash)
        reads_outstanding = true;
        ev_for[si] = (int)si;
        return true;
    }
    bool swept_pair(uint32_t first, uint32_t second) {
        stash_on = false;
        reads_outstanding = true;
        ev_for[first] = (int)second;  // collective_locked(st.si, ev_swept[si], ...)
        ev_for[second] = -1;          // collective_locked(si, nullptr, ...)
        return true;
    }
    bool census_done(uint32_t si, stream X) {  // tt2_sharded_sweep, after the census
        if (!P::record(ev_swept[si], X) || !P::wait(cs, ev_swept[si])) return false;
        if (used[si] && dec_gen[si] > cs_drain_seen) {
            if (!P::wait(cs, ev_drained)) return false;
            cs_drain_seen = drains;
        }
        return true;
    }
    bool gathered(uint32_t si, stream X) { return P::record(ev_ag[si], cs) && P::wait(X, ev_ag[si]); }
    bool before_collective(uint32_t si) {  // collective_locked, first half
        if (ev_for[si] >= 0 && !P::wait(cs, ev_swept[ev_for[si]])) return false;
        if (used[si] && dec_gen[si] > cs_drain_seen) {
            if (!P::wait(cs, ev_drained)) return false;
            cs_drain_seen = drains;
        }
        used[si] = true;
        return true;
    }
    bool after_collective(uint32_t si, size_t &n_drain) {  // collective_locked, second half
        if (!P::record(ev_comb[si], cs)) return false;
        pend[n_pend++] = si;
        n_drain = n_pend > depth ? (group < n_pend ? group : n_pend) : 0;
        return true;
    }
    size_t pending() const { return n_pend; }
    uint32_t pending_slot(size_t i) const { return pend[i]; }
    bool drain_begin(size_t &k) {  // drain_locked
        if (k > n_pend) k = n_pend;
        return k == 0 || P::wait(ds, ev_comb[pend[k - 1]]);
    }
    bool drain_end(size_t k) {
        ++drains;
        for (size_t i = 0; i < k; ++i) dec_gen[pend[i]] = drains;
        if (!P::record(ev_drained, ds)) return false;
        for (size_t i = k; i < n_pend; ++i) pend[i - k] = pend[i];
        n_pend -= k;
        return true;
    }
    bool drained_to(stream s) { return P::record(ev_ds, ds) && P::wait(s, ev_ds); }  // drain_to's tail
    int fence(stream writer) {  // comm_fence_reads
        if (!reads_outstanding) return 0;
        for (uint32_t i = 0; i < kSlots; ++i)
            if (used[i] && !P::wait(writer, ev_swept[i])) return -1;
        reads_outstanding = false;
        return 1;
    }

  private:
    stream ctx{}, cs{}, ds{}, ss[2] = {};
    event ev_swept[kSlots], ev_comb[kSlots], ev_ag[kSlots], ev_in, ev_ctx, ev_drained, ev_ds;
    uint64_t drains = 0, cs_drain_seen = 0;
    bool two_streams, reads_outstanding = false, stash_on = false;
    uint64_t ctx_seen = ~0ull;
    stream ctx_seen_stream = -1;  // (the library's null: no caller stream)
    bool used[kSlots] = {};
    uint64_t dec_gen[kSlots] = {};
    int ev_for[kSlots] = {};
    uint32_t pend[2 * kSlots] = {};
    size_t n_pend = 0;
    uint64_t submitted = 0, x_comb_seen = 0;
    stream x_stream = -1;
    uint32_t depth, group;
};

enum Kind { kKeys, kKeysFlags, kTaint };  // the combine kinds (NU+NN; the resource / NodeAffinity sets; TaintToleration)

struct Setting {
    Kind kind;
    bool two, coalesce;
    uint32_t depth;
};

enum StepKind { kSubmitA, kSubmitB, kDrainA, kDrainB, kTableWrite, kRegrow, kStepKinds };

long failed = 0;
void check(bool ok, const char *what, long k = -1) {
    if (ok) return;
    if (failed++ < 20) std::printf("FAIL %s (k = %ld)\n", what, k);
}

// ms_comm.cpp over a rule and the world it acts on. B: batches a run may submit.
template <template <class> class Rule, int N, int B>
struct Sim {
    using P = Policy<N>;
    World<N> w;
    Rule<P> r;
    Setting set;
    Res<N> table, d_tt, keys[kSlots], mine[kSlots], cen_mine[kSlots], cen_all[kSlots], pods[B], results[B];
    // a batch's payload, as ms_comm.cpp keeps it: queued behind its collective (a later submission
    // may take its slot before its decode is enqueued), or stashed
    struct Batch {
        uint32_t slot;
        int id, X;
    } pend[2 * kSlots] = {}, stash = {};
    size_t n_pend = 0;
    int keys_of[kSlots], mine_of[kSlots];  // the batch whose sweep / collective a slot's buffers hold (-1: none)
    bool has_buffers[kSlots] = {}, grow_next = false;
    bool regrew_pending = false;  // a slot was regrown while its batch was pending
    bool decoded[B] = {}, seen[B] = {};
    int n_batches = 0;
    uint64_t ctx_seq = 0;  // the context's StreamOrder::seq()
    // ms_cycle.cpp tt_take / tt_release (the context's, shared with the single-shard cycles)
    order_model::ModelEvent<N> ev_tt;
    int tt_stream = -1;

    const char *first_bad = nullptr;  // the first access that broke the invariant

    explicit Sim(const Setting &s) : r(s.depth, s.two), set(s) {
        r.attach(kCtx, kColl, kDec, kSweep0, kSweep1);
        for (uint32_t i = 0; i < kSlots; ++i) keys_of[i] = mine_of[i] = -1;
    }
    // What a collective or a decode reads must be what its own batch's sweep or collective wrote.
    void holds(int have, int want, const char *what) {
        if (have == want) return;
        w.violated = true;
        if (!first_bad) first_bad = what;
    }

    void access(int s, Res<N> &res, bool write, const char *what) {
        w.access(s, res, write);
        if (w.violated && !first_bad) first_bad = what;
    }

    bool coalescable() const { return set.coalesce && !set.two && set.kind == kKeys; }

    bool drain_locked(size_t k) {
        if (!r.drain_begin(k)) return false;
        if (k == 0) return true;
        for (size_t i = 0; i < k; ++i) {
            const uint32_t si = pend[i].slot;
            const int b = pend[i].id;
            if (si != r.pending_slot(i)) w.violated = true;  // (the payload queue and the class's ring move together)
            access(kDec, mine[si], false, "mine read on kDec");
            holds(mine_of[si], b, "the decode reads another batch's reduced keys");
            access(kDec, pods[b], false, "pods read on kDec");
            if (set.kind == kTaint) access(kDec, cen_all[si], false, "cen_all read on kDec");
            access(kDec, results[b], true, "results written on kDec");
            decoded[b] = true;
        }
        if (!r.drain_end(k)) return false;
        for (size_t i = k; i < n_pend; ++i) pend[i - k] = pend[i];
        n_pend -= k;
        return true;
    }
    bool collective(const Batch &bt) {
        const uint32_t si = bt.slot;
        if (!r.before_collective(si)) return false;
        access(kColl, keys[si], false, "keys read on kColl");
        holds(keys_of[si], bt.id, "the collective reads another batch's keys");
        access(kColl, mine[si], true, "mine written on kColl");
        mine_of[si] = bt.id;
        size_t n_drain = 0;
        if (!r.after_collective(si, n_drain)) return false;
        pend[n_pend++] = bt;
        return n_drain == 0 || drain_locked(n_drain);
    }
    void sweep(const Batch &bt) {
        const uint32_t si = bt.slot;
        const int X = bt.X;
        access(X, table, false, "table read on X");
        access(X, pods[bt.id], false, "pods read on X");
        access(X, keys[si], true, "keys written on X");
        keys_of[si] = bt.id;
    }
    bool flush_stash() {
        if (!r.held()) return true;
        const Batch bt = stash;
        sweep(bt);
        if (!P::record(r.sweep_event(bt.slot), bt.X)) return false;  // (the dispatch's own)
        return r.swept(bt.slot, bt.X, true) && collective(bt);
    }
    // ms_cycle.cpp tt_take / tt_release: the context's hand-off of d_tt, not the class's (no failure
    // is injected into it)
    void tt_take(int X) {
        const long f = w.fail_in;
        w.fail_in = 0;
        if (tt_stream >= 0 && tt_stream != X) P::wait(X, ev_tt);
        w.fail_in = f;
    }
    void tt_release(int X) {
        const long f = w.fail_in;
        w.fail_in = 0;
        P::record(ev_tt, X);
        tt_stream = X;
        w.fail_in = f;
    }
    bool tt2_sweep(const Batch &bt) {
        const uint32_t si = bt.slot;
        const int b = bt.id, X = bt.X;
        tt_take(X);
        const bool ok = [&] {
            access(X, d_tt, true, "d_tt written on X");  // the planes and the census
            access(X, table, false, "table read on X");
            access(X, pods[b], false, "pods read on X");
            access(X, cen_mine[si], true, "cen_mine written on X");
            if (!r.census_done(si, X)) return false;
            access(kColl, cen_mine[si], false, "cen_mine read on kColl");
            access(kColl, cen_all[si], true, "cen_all written on kColl");
            if (!r.gathered(si, X)) return false;
            access(X, d_tt, true, "d_tt written on X");  // the picks
            access(X, table, false, "table read on X");
            access(X, pods[b], false, "pods read on X");
            access(X, cen_all[si], false, "cen_all read on X");
            access(X, keys[si], true, "keys written on X");
            keys_of[si] = b;
            return true;
        }();
        tt_release(X);  // (after a failure too)
        return ok && r.swept(si, X, false);
    }
    bool submit(int s) {
        if (n_batches == B) {
            w.overflow = true;
            return false;
        }
        const int b = n_batches++;
        access(s, pods[b], true, "pods written on s");  // (the caller's, before the call)
        const bool co = coalescable();
        if (!co && !flush_stash()) return false;
        const uint32_t si = r.next_slot();
        if (grow_next || !has_buffers[si]) {  // slot_ensure
            for (size_t i = 0; i < n_pend; ++i) regrew_pending |= pend[i].slot == si;
            if (const size_t k = r.pending_through(si))
                if (!drain_locked(k)) return false;
            if (has_buffers[si]) w.device_sync();  // (the release of the old blocks waits for the device)
            if (!r.regrown(si)) return false;
            keys[si] = mine[si] = cen_mine[si] = cen_all[si] = Res<N>();
            keys_of[si] = mine_of[si] = -1;
            has_buffers[si] = true;
            grow_next = false;
        }
        int X = -1;
        if (!r.begin(s, ctx_seq, co, X)) return false;
        const Batch bt{si, b, X};
        if (co && (!r.held() || stash.X != X)) {
            if (!flush_stash()) return false;
            stash = bt;
            r.hold(si);
            return true;
        }
        if (co) {  // the stashed batch and this one in one launch
            const Batch b0 = stash;
            const uint32_t s0 = b0.slot;
            access(X, table, false, "table read on X");
            access(X, pods[b0.id], false, "pods read on X");
            access(X, pods[b], false, "pods read on X");
            access(X, keys[s0], true, "keys written on X");
            access(X, keys[si], true, "keys written on X");
            keys_of[s0] = b0.id;
            keys_of[si] = b;
            if (!P::record(r.sweep_event(si), X)) return false;
            return r.swept_pair(s0, si) && collective(b0) && collective(bt);
        }
        if (set.kind == kTaint) {
            if (!tt2_sweep(bt)) return false;
        } else {
            sweep(bt);
            if (!P::record(r.sweep_event(si), X) || !r.swept(si, X, true)) return false;
        }
        return collective(bt);
    }
    bool drain_to(int s) {
        if (!flush_stash() || !drain_locked(r.pending()) || !r.drained_to(s)) return false;
        for (int b = 0; b < n_batches; ++b)
            if (decoded[b] && !seen[b]) {
                access(s, results[b], false, "results read on s");
                seen[b] = true;
            }
        return true;
    }
    bool table_write() {  // flush_locked: the fence, the deltas on the context stream, wrote_ctx
        if (!flush_stash()) return false;  // comm_fence_reads
        if (r.fence(kCtx) < 0) return false;
        access(kCtx, table, true, "table written on kCtx");
        ++ctx_seq;
        return true;
    }
    bool step(int kind) {
        order_model::world<N, kStreams>() = &w;
        switch (kind) {
        case kSubmitA: return submit(kA);
        case kSubmitB: return submit(kB);
        case kDrainA: return drain_to(kA);
        case kDrainB: return drain_to(kB);
        case kTableWrite: return table_write();
        default: grow_next = true; return true;  // the next submission's slice outgrows its slot
        }
    }
};

// Both rules over one sequence; the counts must agree while the parent's rule
// still holds the invariant.
template <int N, int B>
struct Pair {
    Sim<ShardOrder, N, B> a;
    Sim<ParentShard, N, B> b;
    const char *parent_bad = nullptr;  // the access at which the parent rule first broke the invariant
    bool reported_ = false;
    char trace_[3 * 200 + 1] = "";  // the steps so far, for a failure's report
    int n_trace_ = 0;
    explicit Pair(const Setting &s) : a(s), b(s) {}
    void step(int kind, long k = -1) {
        if (n_trace_ < 199) {
            trace_[3 * n_trace_] = ' ';
            trace_[3 * n_trace_ + 1] = "ABabWG"[kind];
            trace_[3 * n_trace_ + 2] = ' ';
            trace_[3 * n_trace_ + 3] = 0;
            ++n_trace_;
        }
        check(a.step(kind), "the class reported a failure the model never injected", k);
        if (a.w.violated && !reported_) {
            reported_ = true;
            check(false, "invariant: an access does not follow an earlier conflicting one:", k);
            if (failed <= 20) std::printf("  %s; kind %d, two streams %d, coalescing %d, depth %u; steps:%s\n", a.first_bad, (int)a.set.kind,
                        (int)a.set.two, (int)a.set.coalesce, a.set.depth, trace_);
        }
        check(!a.w.bad_wait, "wait for an event never recorded", k);
        check(!a.w.overflow, "the model ran out of ids or batches", k);
        check(a.w.events_made <= 3 * (a.set.depth + 1) + 4 + 1, "more events than 3 per slot in use, 4 and ev_tt", k);
        if (b.w.violated) return;  // (nothing left to compare with in this sequence)
        check(b.step(kind), "the parent rule reported a failure the model never injected", k);
        if (b.w.violated && !parent_bad) {
            parent_bad = b.first_bad;
            // the one hole of the parent rule (named_cases): a slot regrown while its batch was pending
            check(b.regrew_pending && b.set.coalesce, "the parent rule breaks the invariant somewhere else", k);
        }
        if (!b.w.violated)
            check(a.w.waits == b.w.waits && a.w.records == b.w.records,
                  "waits / records differ from the parent rule where that rule held the invariant", k);
    }
};

const Kind kKinds[] = {kKeys, kKeysFlags, kTaint};

// Every setting that differs in what the pipeline does (coalescing applies to
// keys-only sweeps on one sweep stream).
template <class F>
void for_each_setting(F f) {
    for (uint32_t depth = 1; depth <= 7; ++depth)
        for (Kind kind : kKinds)
            for (int two = 0; two < 2; ++two)
                for (int co = 0; co < (kind == kKeys && !two ? 2 : 1); ++co) f(Setting{kind, two != 0, co != 0, depth});
}

long nodes = 0, parent_violations = 0;

constexpr int kSearchLen = 7;
using SearchPair = Pair<3, kSearchLen>;  // (7 submits of at most 20 ids each)

// Every sequence of at most `left` more steps after the state in p.
void search(const SearchPair &p, int left) {
    if (left == 0) return;
    for (int kind = 0; kind < kStepKinds; ++kind) {
        SearchPair q = p;
        q.step(kind, nodes);
        ++nodes;
        if (q.b.w.violated && !p.b.w.violated) ++parent_violations;
        search(q, left - 1);
    }
}

template <int N, int B>
void run(Pair<N, B> &p, const int *steps, int n) {
    for (int i = 0; i < n; ++i) p.step(steps[i], i);
}

void named_cases() {
    const Setting lib{kKeys, false, true, 4};  // the library's: depth 4, one sweep stream, coalescing
    {  // the coalesced pair followed by a table write: the fence covers both halves through the second's event
        Pair<4, 16> p(lib);
        const int s[] = {kSubmitA, kSubmitA, kTableWrite, kSubmitA, kSubmitA, kSubmitA, kTableWrite, kDrainA};
        run(p, s, 3);
        check(!p.b.w.violated, "pair + table write: parent rule holds");
        // in: the context wait; the pair: one sweep event, one wait of the collective stream, two collectives;
        // the fence: one wait per used slot
        check(p.a.w.records == 1 + 1 + 2 && p.a.w.waits == 1 + 1 + 2, "pair + table write: 4 records, 4 waits");
        run(p, s + 3, 5);  // (a pair, then a single flushed by the fence)
        check(!p.a.w.violated && !p.b.w.violated, "pairs and a single around table writes");
    }
    {  // a drain between the two halves of a would-be pair: each goes alone
        Pair<4, 16> p(lib);
        const int s[] = {kSubmitA, kDrainA, kSubmitA, kDrainA, kSubmitA, kSubmitA, kDrainA};
        run(p, s, 7);
        check(!p.a.w.violated && !p.b.w.violated, "drain between the halves of a pair");
        check(p.a.r.pending() == 0 && !p.a.r.held(), "drain between the halves: nothing left pending");
    }
    for (int two = 0; two < 2; ++two) {  // alternating caller streams on TaintToleration: d_tt passes A -> B -> A
        Pair<8, 16> p(Setting{kTaint, two != 0, false, 4});
        for (int i = 0; i < 12; ++i) p.step(i & 1 ? kSubmitB : kSubmitA, i);
        p.step(kTableWrite);
        p.step(kDrainB);
        check(!p.a.w.violated && !p.b.w.violated, "TaintToleration, alternating caller streams");
    }
    for (Kind kind : kKinds) {  // a regrown slot in the second round, then a table write
        Pair<8, 16> p(Setting{kind, false, kind == kKeys, 4});
        for (int i = 0; i < 7; ++i) p.step(i % 3 ? kSubmitA : kSubmitB, i);
        p.step(kRegrow);
        for (int i = 0; i < 6; ++i) p.step(i % 3 ? kSubmitB : kSubmitA, i);
        p.step(kTableWrite);
        p.step(kSubmitA);
        p.step(kDrainA);
        check(!p.a.w.violated && !p.b.w.violated, "regrown slot");
    }
    {  // the hole of the parent rule: with a submission held, the next one's slot comes round while its
       // batch is still pending (2 pending + the held one + the new one = depth + 2 at depth 2); regrown
       // there, the pending decode reads the new buffers. The class drains that batch first: one wait
       // and one record more than the parent, which the later drain no longer spends on it.
        Pair<4, 16> p(Setting{kKeys, false, true, 2});
        const int s[] = {kSubmitA, kSubmitA, kSubmitA, kRegrow};
        run(p, s, 4);  // (a pair: two pending; one held)
        check(!p.b.w.violated && p.b.r.pending() == 2 && p.b.r.held(), "regrown pending slot: two pending, one held");
        const long waits = p.b.w.waits, records = p.b.w.records;
        check(p.a.w.waits == waits && p.a.w.records == records, "regrown pending slot: equal counts before it");
        p.step(kSubmitA);
        check(!p.a.w.violated, "regrown pending slot: the class drains the slot's batch first");
        check(p.b.w.violated, "regrown pending slot: the parent rule is expected to fail (the model must see it)");
        Pair<4, 16> q(Setting{kKeys, false, true, 2});  // the same without the regrow: what the submit costs alone
        run(q, s, 3);
        q.step(kSubmitA);
        check(!q.b.w.violated, "held submission, slot still pending, no regrow: the parent rule holds");
        check(p.a.w.waits == p.b.w.waits + 1 && p.a.w.records == p.b.w.records + 1,
              "regrown pending slot: one wait and one record more than the parent rule spends on the same submit");
    }
    // a failed record or wait at each position of one submit (the 8th: slots in their second round): the
    // class reports it, and the next submit and a drain still hold the invariant
    for (Kind kind : kKinds)
        for (int co = 0; co < (kind == kKeys ? 2 : 1); ++co) {
            Sim<ShardOrder, 8, 16> base(Setting{kind, false, co != 0, 4});
            for (int i = 0; i < 7; ++i) check(base.step(i & 1 ? kSubmitB : kSubmitA), "warm-up submit");
            Sim<ShardOrder, 8, 16> whole = base;
            whole.w.fail_in = 1000;  // (counts the records and waits a failure can be injected into)
            check(whole.step(kSubmitA), "the submit without a failure");
            const long ops = 1000 - whole.w.fail_in;
            check(ops >= 2, "a submit records and waits");
            for (long k = 1; k <= ops; ++k) {
                Sim<ShardOrder, 8, 16> f = base;
                f.w.fail_in = k;
                check(!f.step(kSubmitA), "the class reports the failed record or wait", k);
                check(f.w.fail_in == 0, "the failure was met", k);
                check(f.step(kSubmitB) && !f.w.violated, "after a failed submit the next one holds the invariant", k);
                if (f.w.violated && failed <= 20) std::printf("  %s (kind %d, coalescing %d)\n", f.first_bad, (int)kind, co);
                check(f.step(kDrainA) && !f.w.violated && !f.w.bad_wait, "and so does the drain after it", k);
            }
        }
}

long random_runs = 0;

// Seeded sequences with 40 submissions each (depth 7 has 8 slots: every slot is
// reused at least three times) and other steps between them, every setting in turn.
void random_sequences() {
    std::mt19937 rng(20261020u);
    for (int round = 0; round < 40; ++round)
        for_each_setting([&](const Setting &s) {
            Pair<16, 40> p(s);
            // per sequence its own mix, so that long runs on one stream occur as well as churn
            const unsigned p_b = rng() % 5, p_drain = rng() % 4, p_write = rng() % 4, p_grow = rng() % 3;
            int submits = 0;
            for (long i = 0; submits < 40; ++i) {
                int kind = rng() % 4 < p_b ? kSubmitB : kSubmitA;
                const unsigned other = rng() % 16;
                if (other < p_drain) kind = rng() & 1 ? kDrainA : kDrainB;
                else if (other < p_drain + p_write) kind = kTableWrite;
                else if (other < p_drain + p_write + p_grow) kind = kRegrow;
                submits += kind == kSubmitA || kind == kSubmitB;
                p.step(kind, random_runs);
            }
            p.step(rng() & 1 ? kDrainA : kDrainB, random_runs);
            if (p.b.w.violated) ++parent_violations;
            ++random_runs;
        });
}

}  // namespace

int main() {
    named_cases();
    long settings = 0;
    for_each_setting([&](const Setting &s) {
        search(SearchPair(s), kSearchLen);
        ++settings;
    });
    std::printf("sequences up to length %d checked: %ld in %ld settings (the parent rule first breaks the invariant in %ld)\n",
                kSearchLen, nodes, settings, parent_violations);
    check(nodes == settings * (6 + 36 + 216 + 1296 + 7776 + 46656 + 279936), "search size");
    const long in_search = parent_violations;
    parent_violations = 0;
    random_sequences();
    std::printf("random sequences of 40 submissions checked: %ld (the parent rule breaks the invariant in %ld)\n",
                random_runs, parent_violations);
    check(in_search > 0 && parent_violations > 0, "both searches meet the regrown pending slot, where the parent rule fails");
    std::printf("%ld failed\n", failed);
    return failed ? 1 : 0;
}
