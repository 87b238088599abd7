// A model of streams and events for the ordering classes
// (mini-kube-scheduler_amd/csrc/ms_order.h, ms_shard_order.h), shared by
// test_order.cpp and test_shard_order.cpp. Streams are small integers, every
// enqueued piece of work gets an id, and a stream carries the set of ids that
// happen before its tail: record snapshots that set into the event, wait
// unions the snapshot into the stream. Two invariants can be checked on it:
// a total order (work / fence: every piece of work follows every ordered one
// enqueued before it) and a per-resource one (access: every access follows
// every earlier conflicting access to the same resource).
#pragma once

#include <cstdint>

namespace order_model {

template <int N>
struct Bits {
    uint64_t w[N] = {};
    void set(int i) { w[i >> 6] |= 1ull << (i & 63); }
    void merge(const Bits &o) {
        for (int k = 0; k < N; ++k) w[k] |= o.w[k];
    }
    bool holds(const Bits &o) const {
        for (int k = 0; k < N; ++k)
            if (o.w[k] & ~w[k]) return false;
        return true;
    }
};

template <int N>
struct ModelEvent {
    bool made = false;  // created lazily, by the first record
    Bits<N> snap;
};

// What touched a resource so far: two reads do not conflict, everything else does.
template <int N>
struct Resource {
    Bits<N> all, writes;
};

// The device as a protocol sees it (S streams, at most 64 N pieces of work),
// and what the checks count. Stream 0 is the context stream.
template <int N, int S>
struct World {
    Bits<N> hb[S];    // per stream: the work that happens before its tail
    Bits<N> ordered;  // every ordered piece of work enqueued so far
    int next_id = 0;
    long records = 0, waits = 0, events_made = 0;
    bool violated = false, bad_wait = false, overflow = false;
    long fail_in = 0;  // the k-th record / wait from now fails (1 = the next one); 0 = none

    int new_id(int s) {
        if (next_id >= 64 * N) {
            overflow = true;
            return 64 * N - 1;
        }
        hb[s].set(next_id);
        return next_id++;
    }
    // A piece of ordered work on stream s: checked, then part of the order.
    void work(int s) {
        if (!hb[s].holds(ordered)) violated = true;
        ordered.set(new_id(s));
    }
    // Waits were inserted into the context stream behind work on another
    // stream: so must everything ordered after it.
    void fence() { ordered.set(new_id(0)); }
    // A read or a write of r on stream s: checked against the earlier
    // conflicting accesses, then one of them.
    void access(int s, Resource<N> &r, bool write) {
        if (!hb[s].holds(write ? r.all : r.writes)) violated = true;
        const int id = new_id(s);
        r.all.set(id);
        if (write) r.writes.set(id);
    }
    // The host waited for the whole device: everything enqueued so far happens
    // before anything enqueued later, on every stream.
    void device_sync() {
        Bits<N> all;
        for (int s = 0; s < S; ++s) all.merge(hb[s]);
        for (int s = 0; s < S; ++s) hb[s] = all;
    }
};

// The policy is stateless, like the library's: it reaches the world of the
// run being stepped through one slot (the driver sets it), so a run, world and
// rule together, can be copied when the search branches.
template <int N, int S>
World<N, S> *&world() {
    static World<N, S> *p = nullptr;
    return p;
}

template <int N, int S>
struct ModelPolicy {
    using stream = int;
    using event = ModelEvent<N>;
    static bool record(event &e, int s) {
        World<N, S> *w = world<N, S>();
        if (w->fail_in && --w->fail_in == 0) return false;
        if (!e.made) {
            e.made = true;
            ++w->events_made;
        }
        e.snap = w->hb[s];
        ++w->records;
        return true;
    }
    static bool wait(int s, event &e) {
        World<N, S> *w = world<N, S>();
        if (w->fail_in && --w->fail_in == 0) return false;
        if (!e.made) w->bad_wait = true;  // (a wait for an event never recorded orders nothing)
        w->hb[s].merge(e.snap);
        ++w->waits;
        return true;
    }
};

}  // namespace order_model
