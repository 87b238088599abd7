"""Node deltas as one model on the GPU: an engine walks the scripts of
tests/_table_model.py beside the model, for every plugin set. After every op
ms_info's two counters equal the model's; after every drain ms_nodes_read over
the whole capacity equals the model field by field (tombstones and rows never
added included), ms_explain's summaries decode to the cycle, and a schedule
(host, compact, ms_select_batch_device, batched or sequential by turns) equals
the oracle on the model's view, bit for bit. tests/test_table_model.py proves on
the CPU that every step of these scripts moves pods and hits the plane, list
or column property it is there for.

Then the parts of the maintenance path no script reaches: the list form of the
K1 sweep on lists that cross a tile edge (it needs chunks of 80 pods and more),
binds between two sequential calls, the refusal of a bind on an absent row, the
table of which entry points drain, and the multi-call shard protocols holding
one table from their first call to their last.
"""
import numpy as np
import pytest

import _explain_ref
import _nam_required_ref as nref
import _table_model as tm
from minisched_amd import _lib, synth
from minisched_amd._lib import MODE_BATCHED, MODE_SEQUENTIAL, Engine
from test_gpu_parity import assert_same, need_gpu  # noqa: F401
from test_gpu_pp_class_runs import _n_pods, _pods

pytestmark = pytest.mark.gpu


class _Gpu:
    def __init__(self):
        import torch

        self.torch, self.dev = torch, torch.device("cuda:0")
        self.stream = torch.cuda.Stream(device=self.dev)
        self.sp = self.stream.cuda_stream

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)
        self.torch.cuda.synchronize()
        return t

    def buf(self, nbytes, fill=0):
        t = self.torch.full((max(1, nbytes),), fill, dtype=self.torch.uint8, device=self.dev)
        self.torch.cuda.synchronize()  # (the fill ran on torch's stream, not ours)
        return t

    def keys(self, g, p):
        t = self.torch.zeros((g, p), dtype=self.torch.int64, device=self.dev)
        self.torch.cuda.synchronize()
        return t

    def get(self, t, dtype):
        self.stream.synchronize()
        return t.cpu().numpy().view(dtype)


def _assert_read(e, m, tag):
    got, want = e.read(m.base, m.cap), m.expected_read()
    for f in _lib.NODE_REC.names:
        if not np.array_equal(got[f], want[f]):
            bad = np.flatnonzero(got[f] != want[f])[:8]
            raise AssertionError(f"{tag}: {f} differs at rows {bad.tolist()}: read {got[f][bad].tolist()} "
                                 f"model {want[f][bad].tolist()}")


def _assert_info(e, m, tag):
    i = e.info()
    assert (i.present_nodes, i.pending_deltas) == (m.present, m.pending), tag


class Driver:
    """The engine beside the model in tm.walk()."""

    def __init__(self, script, ps, oracle, big=None):
        self.script, self.ps, self.oracle, self.big = script, ps, oracle, big
        self.gpu = _Gpu()
        self.e = Engine(max_nodes=script.cap, plugin_set=ps, node_base=script.node_base, seed=script.seed,
                        score_weights=tm.WEIGHTS.get(ps, (0, 0)))
        if ps == 4:
            ts, rq = tm.nam_tables(script.seed)
            self.e.nam_term_sets_ext(ts)
            self.e.nam_required_sets(rq)

    def op(self, m, op, refused):
        e = self.e
        if op[0] in ("U", "BADU"):
            if refused:
                with pytest.raises(_lib.MSError) as err:
                    e.upsert(op[1], op[2])
                assert err.value.code == _lib.MS_E_CAPACITY
            else:
                e.upsert(op[1], op[2])
        elif op[0] == "D":
            e.delete(op[1])
        elif op[0] == "C":
            e.commit_bind(int(op[1]), op[2])
        else:
            e.uncommit_bind(int(op[1]), op[2])
        _assert_info(e, m, f"{self.script}: after {op[0]}")  # (pending before the drain, present at once)

    def drained(self, m, k, st):
        self.e.flush()
        _assert_info(self.e, m, f"{self.script} step {k}: after the drain")
        _assert_read(self.e, m, f"{self.script} step {k} ({st.why})")

    def _run(self, form, pods):
        e = self.e
        if form == "compact":
            return e.schedule_compact(_lib.compact_pods(pods))
        if form == "device":
            g = self.gpu
            d, out = g.put(pods), g.buf(24 * len(pods), 0xCD)
            e.select_batch_device(len(pods), d.data_ptr(), out.data_ptr(), g.sp)
            return g.get(out, _lib.RESULT)
        return e.schedule(pods, MODE_SEQUENTIAL if form == "sequential" else MODE_BATCHED)

    def schedule(self, m, k, st, form, pods, want, batched):
        tag = f"{self.script} step {k} ({st.why}), {form}"
        head = pods[:_lib.EXPLAIN_MAX_PODS]
        _, sums = self.e.explain(head, rows=False)
        assert (sums["present"] == m.present).all(), tag
        for j in range(len(head)):
            got = _explain_ref.decode(sums[j])
            assert got == (batched["node"][j], batched["score"][j], batched["code"][j], batched["mask"][j]), (tag, j)
        try:
            assert_same(self._run(form, pods), want)
        except AssertionError as err:
            raise AssertionError(f"{tag}: {err}") from None
        if self.big is not None:  # the list form needs chunks of 80 pods and more
            o = self.oracle.schedule_nunn_omp(m.oracle_view(), self.big, seed=self.script.seed,
                                              node_base=self.script.node_base)
            try:
                assert_same(self.e.schedule(self.big, MODE_BATCHED), o)
            except AssertionError as err:
                raise AssertionError(f"{tag}, the large batch: {err}") from None
            self._big_want = o

    def scheduled(self, m, k, st):
        if self.big is not None:
            m.apply_results(self.big, self._big_want)
        _assert_read(self.e, m, f"{self.script} step {k}: the bound columns")
        _assert_info(self.e, m, f"{self.script} step {k}: after the cycle")

    def close(self):
        self.e.close()


def _walk(script, ps, oracle, big=None):
    d = Driver(script, ps, oracle, big)
    try:
        return tm.walk(script, ps, oracle, d)
    finally:
        d.close()


@pytest.mark.parametrize("ps", range(5))
@pytest.mark.parametrize("idx", range(len(tm.directed_scripts())))
def test_directed_scripts(oracle, idx, ps):
    script = tm.directed_scripts()[idx]
    log = _walk(script, ps, oracle)
    assert all(value == st.expect for st, value, _, _ in log)


@pytest.mark.parametrize("ps", range(5))
@pytest.mark.parametrize("seed", tm.RANDOM_SEEDS)
def test_random_scripts(oracle, seed, ps):
    _walk(tm.random_script(seed), ps, oracle)


def test_list_lengths_in_the_list_form(oracle, monkeypatch):
    # the list script again with, beside its 320 pods, a batch whose chunks form class runs
    # (tests/test_gpu_pp_class_runs.py): only those sweep the candidate lists, so only
    # they see a list k_build_cand did not rebuild, or rebuilt a tile short
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    script = tm.list_script()
    log = _walk(script, 0, oracle, big=_pods(_n_pods(), script.seed))
    assert [v for _, v, _, _ in log][1:4] == [(193, 11), (192, 12), (191, 13)]


# ---- binds ---------------------------------------------------------------------------------
def test_binds_between_sequential_calls(oracle):
    # commits and uncommits between sequential calls on one engine: all five columns, on a node
    # with Requested of its own, with a pod of 2^44 a column; the next call must see them in
    # the engine's derived rows (it equals the oracle on the model's columns, and the bound
    # node no longer takes the pod it was about to take)
    seed, n, ps = 7, 2100, 1
    recs = tm.base_records(n, 0, seed)
    m = tm.TableModel(n)
    calls = [tm.pods_for(ps, 320, seed, start=1000 * k) for k in range(4)]

    def cycle(e, pods, tag):
        m.drain()  # (as the call does)
        want = tm.oracle_results(oracle, ps, m.oracle_view(), pods, seed, 0, sequential=True)
        try:
            assert_same(e.schedule(pods, MODE_SEQUENTIAL), want)
        except AssertionError as err:
            raise AssertionError(f"{tag}: {err}") from None
        m.apply_results(pods, want)
        _assert_read(e, m, tag)

    with Engine(max_nodes=n, plugin_set=ps, seed=seed) as e:
        # the node: so much larger than the rest that, Requested and all, LeastAllocated puts it
        # first for every pod of its digit, call after call, while NodeResourcesFit lets it
        t = int(np.flatnonzero(recs["unschedulable"] == 0)[0])
        recs[t] = tm._with(recs[t], req_milli_cpu=700, req_memory=1 << 30, nonzero_milli_cpu=700,
                           nonzero_memory=1 << 30, pod_count=3, alloc_milli_cpu=640_000, alloc_memory=1280 << 30)
        e.upsert(np.arange(n), recs)
        m.upsert(np.arange(n), recs)
        cycle(e, calls[0], "first call")
        unbound = tm.oracle_results(oracle, ps, m.oracle_view(), calls[1], seed, 0, sequential=True)
        binds = [tm.bind_pod(1), tm.bind_pod(2), tm.bind_pod(3, huge=True)]
        for p in binds:
            e.commit_bind(t, p)
            m.commit(t, p)
            _assert_read(e, m, "after a commit")
        assert m.recs["req_memory"][t] > 1 << 44 and m.recs["pod_count"][t] >= 6
        bound = tm.oracle_results(oracle, ps, m.oracle_view(), calls[1], seed, 0, sequential=True)
        assert (unbound["node"] == t).any() and not (bound["node"] == t).any()  # the binds change the cycle
        cycle(e, calls[1], "second call, after three commits")
        e.uncommit_bind(t, binds[2])
        m.uncommit(t, binds[2])
        _assert_read(e, m, "after the uncommit")
        cycle(e, calls[2], "third call, after the uncommit")
        # a commit and its uncommit: every column and the next call as if neither had happened
        before = e.read(0, n)
        for p in (tm.bind_pod(4, huge=True), tm.bind_pod(5)):
            e.commit_bind(t, p)
            e.uncommit_bind(t, p)
        assert e.read(0, n).tobytes() == before.tobytes()
        cycle(e, calls[3], "fourth call, after a commit and its uncommit")
        with pytest.raises(_lib.MSError) as err:  # (as test_gpu_parity.py::test_commit_uncommit)
            e.commit_bind(n + 5, binds[0])
        assert err.value.code == _lib.MS_E_CAPACITY


def test_bind_on_absent_row_is_refused():
    # a tombstone and a row never added: MS_E_INVAL with a message, the table untouched
    m = tm.TableModel(12, node_base=40)
    recs = tm.base_records(10, 40, 3)
    pod = tm.bind_pod(1)
    with Engine(max_nodes=12, plugin_set=1, node_base=40, seed=3) as e:
        for x in (e, m):
            x.upsert(np.arange(40, 50), recs)
            x.delete([43])
        m.drain()
        e.flush()
        for o in (43, 51):
            for call, mcall in ((e.commit_bind, m.commit), (e.uncommit_bind, m.uncommit)):
                with pytest.raises(_lib.MSError) as err:
                    call(o, pod)
                assert err.value.code == _lib.MS_E_INVAL and "not present" in str(err.value)
                with pytest.raises(tm.AbsentRow):
                    mcall(o, pod)
                _assert_read(e, m, f"after the refused bind on {o}")
        # a delete still queued when the bind arrives: the bind drains, then refuses
        for x in (e, m):
            x.delete([44])
        with pytest.raises(_lib.MSError):
            e.commit_bind(44, pod)
        with pytest.raises(tm.AbsentRow):
            m.commit(44, pod)
        _assert_info(e, m, "after the refused bind on a row deleted in the same drain")
        _assert_read(e, m, "the same")
        e.commit_bind(45, pod)  # (and a present row still binds)
        m.commit(45, pod)
        _assert_read(e, m, "a bind on a present row")


# ---- who drains ------------------------------------------------------------------------------
def _drain_case(e, base, name, call, drains, gpu):
    """One upsert that rewrites a row with its identical record, then the entry point:
    pending_deltas is 0 after one that drains, still 1 after one that does not."""
    e.upsert([base], e.read(base, 1))
    assert e.info().pending_deltas == 1, name
    call()
    gpu.stream.synchronize()
    assert e.info().pending_deltas == (0 if drains else 1), f"{name} {'did not drain' if drains else 'drained'}"
    e.flush()


def test_drain_table(oracle):
    g = _Gpu()
    n, P, seed = 200, 64, 5
    recs = tm.base_records(n, 0, seed)
    pod = tm.bind_pod(2)
    seen = set()

    def case(e, name, call, drains):
        seen.add(name)
        _drain_case(e, 0, name, call, drains, g)

    def engine(ps):
        e = Engine(max_nodes=n, plugin_set=ps, seed=seed)
        e.upsert(np.arange(n), recs)
        e.flush()
        return e

    with engine(0) as e:
        pr = tm.pods_for(0, P, seed)
        pods, keys, out = g.put(pr), g.buf(8 * P), g.buf(24 * P)
        rows, sums = g.buf(24 * 8 * n), g.buf(32 * 8)
        case(e, "ms_nodes_flush", e.flush, True)
        case(e, "ms_nodes_read", lambda: e.read(3, 2), True)
        case(e, "ms_commit_bind", lambda: e.commit_bind(7, pod), True)
        case(e, "ms_uncommit_bind", lambda: e.uncommit_bind(7, pod), True)
        case(e, "ms_schedule_batch", lambda: e.schedule(pr), True)
        case(e, "ms_schedule_batch_compact", lambda: e.schedule_compact(_lib.compact_pods(pr)), True)
        case(e, "ms_sweep_device", lambda: e.sweep_device(P, pods.data_ptr(), keys.data_ptr(), 0, g.sp), True)
        case(e, "ms_select_batch_device", lambda: e.select_batch_device(P, pods.data_ptr(), out.data_ptr(), g.sp), True)
        case(e, "ms_schedule_sequential_device",
             lambda: e.schedule_sequential_device(P, pods.data_ptr(), out.data_ptr(), g.sp), True)
        case(e, "ms_explain", lambda: e.explain(pr[:8]), True)
        case(e, "ms_explain_device",
             lambda: e.explain_device(8, pods.data_ptr(), 0, n, rows.data_ptr(), sums.data_ptr(), g.sp), True)
        case(e, "ms_decode_device",
             lambda: e.decode_device(P, pods.data_ptr(), keys.data_ptr(), 0, n, out.data_ptr(), g.sp), False)
        case(e, "ms_decode_device_jobs",
             lambda: e.decode_device_jobs([(P, pods.data_ptr(), keys.data_ptr(), 0, out.data_ptr())], n, g.sp), False)
        case(e, "ms_apply_binds_device", lambda: e.apply_binds_device(P, pods.data_ptr(), out.data_ptr(), g.sp), False)
        case(e, "ms_get_info", e.info, False)
        case(e, "ms_seq_counters", e.seq_counters, False)
        case(e, "ms_last_call_profile", e.last_call_profile, False)
    with engine(1) as e:
        pr = tm.pods_for(1, P, seed)
        pods, out = g.put(pr), g.buf(24 * P)
        cands, flags = g.buf(_lib.SEQ_CAND.itemsize * _lib.SEQ_TOPK * P), g.buf(4 * P)
        done = g.buf(4)
        case(e, "ms_seq_candidates_device",
             lambda: e.seq_candidates_device(P, pods.data_ptr(), cands.data_ptr(), flags.data_ptr(), g.sp), True)
        case(e, "ms_seq_validate_device",
             lambda: e.seq_validate_device(P, pods.data_ptr(), 1, cands.data_ptr(), flags.data_ptr(), out.data_ptr(),
                                           done.data_ptr(), g.sp), False)
    with engine(3) as e:
        pr = tm.pods_for(3, P, seed)
        pods, out, keys = g.put(pr), g.buf(24 * P), g.buf(8 * P)
        summ, census = g.buf(_lib.TT_SUMMARY_BYTES * P), g.buf(_lib.TT_CENSUS_BYTES * P)
        case(e, "ms_tt_summaries_device", lambda: e.tt_summaries_device(P, pods.data_ptr(), summ.data_ptr(), g.sp), True)
        case(e, "ms_tt_decode_device",
             lambda: e.tt_decode_device(P, pods.data_ptr(), 1, summ.data_ptr(), out.data_ptr(), g.sp), False)
        case(e, "ms_tt_census_device", lambda: e.tt_census_device(P, pods.data_ptr(), census.data_ptr(), g.sp), True)
        case(e, "ms_tt_pick_device",
             lambda: e.tt_pick_device(P, pods.data_ptr(), 1, 0, census.data_ptr(), keys.data_ptr(), g.sp), False)
        case(e, "ms_tt_final_device",
             lambda: e.tt_final_device(P, pods.data_ptr(), 1, census.data_ptr(), keys.data_ptr(), out.data_ptr(), g.sp),
             False)
        assert_same(g.get(out, _lib.RESULT), oracle.schedule_tt(recs, pr, literal=True, seed=seed))
    with engine(4) as e:
        ts, rq = tm.nam_tables(seed)
        e.nam_term_sets_ext(ts)
        e.nam_required_sets(rq)
        pr = tm.pods_for(4, P, seed)
        pods, keys, segs, flags = g.put(pr), g.buf(8 * P), g.buf(_lib.NAM_SEG_BYTES * P), g.buf(4 * P)
        case(e, "ms_nam_segment_device", lambda: e.nam_segment_device(P, pods.data_ptr(), segs.data_ptr(), g.sp), True)
        case(e, "ms_nam_keys_device",
             lambda: e.nam_keys_device(P, pods.data_ptr(), 1, 0, segs.data_ptr(), keys.data_ptr(), g.sp), False)
        case(e, "ms_nam_flags_device", lambda: e.nam_flags_device(P, 1, segs.data_ptr(), flags.data_ptr(), g.sp), False)
    assert len(seen) == 15 + 12  # include/minisched_gpu.h "Who drains": both lists, _compact / _device / _jobs apart


# ---- one cycle, one table ------------------------------------------------------------------
CUTS = (0, 37, 300)


def test_tt_two_pass_holds_one_table(oracle):
    # deltas queued between ms_tt_census_device and ms_tt_pick_device wait for the next cycle:
    # the cycle equals the oracle on the table as it stood at the census, the next one the
    # oracle on the new table, and neither pick nor final drains
    g = _Gpu()
    seed, P, CB = 31, 320, _lib.TT_CENSUS_BYTES
    n, G = CUTS[-1], len(CUTS) - 1
    nr = synth.nodes(n, seed=seed, taints=True)
    pr = tm.pods_for(3, P, seed)
    gone = int(np.flatnonzero((nr["unschedulable"][:CUTS[1]] == 0) & (nr["taints"][:CUTS[1]] & 0xFF == 0))[0])
    ten = np.setdiff1d(np.arange(12), [gone])[:10]
    new = nr.copy()
    new["taints"][ten] = np.where(np.arange(10) % 2 == 0, 0, 0x0F00).astype(np.uint32)
    new["allowed_pods"][gone] = -1
    o_old = oracle.schedule_tt(nr, pr, literal=True, seed=seed)
    o_new = oracle.schedule_tt(new, pr, literal=True, seed=seed)
    assert tm.differs(o_old, o_new) > 0
    pods = g.put(pr)
    engines = [Engine(max_nodes=hi - lo, plugin_set=3, node_base=lo, seed=seed) for lo, hi in zip(CUTS[:-1], CUTS[1:])]

    def census():
        c = g.buf(G * P * CB)
        for s, e in enumerate(engines):
            e.tt_census_device(P, pods.data_ptr(), c.data_ptr() + s * P * CB, g.sp)
        return c

    def finish(c, want, tag):
        keys = g.keys(G, P)
        for s, e in enumerate(engines):
            e.tt_pick_device(P, pods.data_ptr(), G, s, c.data_ptr(), keys[s].data_ptr(), g.sp)
        g.stream.synchronize()
        best = keys.max(dim=0).values.contiguous()  # keys < 2^63: the signed max is the unsigned one
        g.torch.cuda.synchronize()
        for s, e in enumerate(engines):
            out = g.buf(24 * P, 0xCD)
            e.tt_final_device(P, pods.data_ptr(), G, c.data_ptr(), best.data_ptr(), out.data_ptr(), g.sp)
            try:
                assert_same(g.get(out, _lib.RESULT), want)
            except AssertionError as err:
                raise AssertionError(f"{tag}, decoded on shard {s}: {err}") from None

    try:
        for e, lo, hi in zip(engines, CUTS[:-1], CUTS[1:]):
            e.upsert(np.arange(lo, hi), nr[lo:hi])
            e.flush()
        c = census()
        g.stream.synchronize()
        engines[0].delete([gone])
        engines[0].upsert(ten, new[ten])
        assert engines[0].info().pending_deltas == 11
        finish(c, o_old, "the cycle whose census preceded the deltas")
        i = engines[0].info()
        assert (i.pending_deltas, i.present_nodes) == (11, CUTS[1] - 1)
        finish(census(), o_new, "the next cycle")
        assert engines[0].info().pending_deltas == 0
    finally:
        for e in engines:
            e.close()


def test_nam_shard_cycle_holds_one_table(oracle):
    # the same for ms_nam_segment_device -> ms_nam_keys_device / ms_nam_flags_device ->
    # ms_decode_device: the labels of the cluster's first non-zero-scoring node change
    # between the calls
    g = _Gpu()
    seed, P, SB = 32, 320, _lib.NAM_SEG_BYTES
    n, G = CUTS[-1], len(CUTS) - 1
    nr = synth.nodes(n, seed=seed, labels=True)
    pr = tm.pods_for(4, P, seed)
    ts, rq = tm.nam_tables(seed)
    pref = nref.decode_preferred(ts)
    scores = lambda z, l: any(w and (zm >> z) & 1 and (lm >> l) & 1 for s in pref for w, zm, lm in s)  # noqa: E731
    f = next(i for i in range(n) if scores(int(nr["zone"][i]), int(nr["label2"][i])))
    new = nr.copy()
    new["zone"][f], new["label2"][f] = (int(nr["zone"][f]) % 8) + 1, 0
    shard = next(s for s in range(G) if CUTS[s] <= f < CUTS[s + 1])
    o_old = nref.schedule_tombstone(oracle, nr, pr, ts, rq, seed=seed, literal=True)
    o_new = nref.schedule_tombstone(oracle, new, pr, ts, rq, seed=seed, literal=True)
    assert tm.differs(o_old, o_new) > 0
    pods = g.put(pr)
    engines = [Engine(max_nodes=hi - lo, plugin_set=4, node_base=lo, seed=seed) for lo, hi in zip(CUTS[:-1], CUTS[1:])]

    def segments():
        sg = g.buf(G * P * SB)
        for s, e in enumerate(engines):
            e.nam_segment_device(P, pods.data_ptr(), sg.data_ptr() + s * P * SB, g.sp)
        return sg

    def finish(sg, want, tag):
        keys, flags, out = g.keys(G, P), g.buf(4 * P, 0xFF), g.buf(24 * P, 0xCD)
        for s, e in enumerate(engines):
            e.nam_keys_device(P, pods.data_ptr(), G, s, sg.data_ptr(), keys[s].data_ptr(), g.sp)
        engines[-1].nam_flags_device(P, G, sg.data_ptr(), flags.data_ptr(), g.sp)
        g.stream.synchronize()
        best = keys.max(dim=0).values.contiguous()
        g.torch.cuda.synchronize()
        present = sum(int(e.info().present_nodes) for e in engines)
        engines[0].decode_device(P, pods.data_ptr(), best.data_ptr(), flags.data_ptr(), present, out.data_ptr(), g.sp)
        try:
            nref.same(g.get(out, _lib.RESULT), want, tag)
        except AssertionError as err:
            raise AssertionError(f"{tag}: {err}") from None

    try:
        for e, lo, hi in zip(engines, CUTS[:-1], CUTS[1:]):
            e.nam_term_sets_ext(ts)
            e.nam_required_sets(rq)
            e.upsert(np.arange(lo, hi), nr[lo:hi])
            e.flush()
        sg = segments()
        g.stream.synchronize()
        engines[shard].upsert([f], new[[f]])
        finish(sg, o_old, "the cycle whose records preceded the delta")
        assert engines[shard].info().pending_deltas == 1
        finish(segments(), o_new, "the next cycle")
        assert engines[shard].info().pending_deltas == 0
    finally:
        for e in engines:
            e.close()
