"""MS_PLUGINS_NU_NN_NAM inside the library on joined contexts (ms_comm.cpp
nam_sharded_sweep), through the loopback build at world 2/3/4/8: this shard's
class records, ONE all-gather of them (nam_class_cap(n, n_sets) records per
rank, not one per pod), the keys pass resuming from the first pass's scratch,
keys (uint64 MAX) and filter bytes (uint8 MAX = OR) reduce-scattered, the slice
decode with NodeAffinity's FitError bit.

Every case is compared, element for element in node, code, score and mask,
with tests/_nam_required_ref.py's schedule_tombstone over the WHOLE cluster
(itself checked against the literal restatement by tests/test_nam_required.py).
Inputs are tests/_nam_required_cases.py's; both tables are registered on every
rank before ms_comm_init, which is the caller's contract (minisched_gpu.h).
"""
import numpy as np
import pytest

import _nam_required_cases as cases
import _nam_required_ref as ref
from minisched_amd import _lib, sharded, synth
from test_gpu_loopback import _cuts, lb, run_ranks  # noqa: F401  (lb: the loopback library fixture)

pytestmark = pytest.mark.gpu

NAM = _lib.PLUGINS_NU_NN_NAM
NO_REQ = _lib.nam_required_sets_array([])
RANK_TIMEOUT = 300

_REFS = {}


def _want(oracle, key, nr, pr, ts, rq, seed, weights=(1, 1), dead=()):
    """The reference, computed once per key and shared (never modified)."""
    if key not in _REFS:
        _REFS[key] = ref.schedule_tombstone(oracle, nr, pr, ts, rq, weights=weights, seed=seed, dead=dead)
    return _REFS[key]


def _classes(pr, n_sets):
    sid = ref.set_id(pr)
    sid = np.where(sid > n_sets, 0, sid)
    return len(set(zip(sid.tolist(), (pr["tolerates_unschedulable"] != 0).tolist())))


def _engine(lib, nr, lo, hi, ts, rq, seed, dead=(), weights=(0, 0), upsert=True):
    e = _lib.Engine(max_nodes=max(1, hi - lo), plugin_set=NAM, node_base=lo, seed=seed, score_weights=weights, lib=lib)
    if ts is not None:
        e.nam_term_sets_ext(ts)
    if rq is not None:
        e.nam_required_sets(rq)
    if upsert and hi > lo:
        e.upsert(np.arange(lo, hi), nr[lo:hi])
        gone = np.asarray([d for d in dead if lo <= d < hi], dtype=np.uint32)
        if len(gone):
            e.delete(gone)
    e.flush()
    return e


def _sharded(lib, nr, pr, ts, rq, cuts, seed, dead=(), weights=(0, 0), steps=6, no_upsert=()):
    """ms_sharded_submit x steps + ms_sharded_drain on len(cuts) joined NAM contexts;
    [(first, count, results)] per rank. no_upsert: ranks that never upsert a node."""
    import torch

    G = len(cuts)
    cid = _lib.comm_id_create(lib)
    dev = torch.device("cuda:0")
    host_pods = pr.view(np.uint8).copy()

    def rank_fn(r):
        lo, hi = cuts[r]
        e = _engine(lib, nr, lo, hi, ts, rq, seed, dead, weights, upsert=r not in no_upsert)
        try:
            e.comm_init(cid, r, G)
            first, count = e.sharded_slice(len(pr))
            assert (first, first + count) == sharded.pod_slice(len(pr), r, G)
            pods = torch.from_numpy(host_pods).to(dev)
            res = torch.full((max(1, count) * 24,), 0xAB, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()  # (the copy and the fill ran on torch's stream, not the library's)
            s = torch.cuda.Stream(device=dev)
            for _ in range(steps):  # more than the pipeline depth: slots are reused after their decodes
                e.sharded_submit(len(pr), pods.data_ptr(), res.data_ptr(), s.cuda_stream)
            e.sharded_drain(s.cuda_stream)
            s.synchronize()
            torch.cuda.synchronize()
            return first, count, res.cpu().numpy().view(_lib.RESULT)[:count].copy()
        finally:
            e.close()

    return run_ranks(G, rank_fn, timeout=RANK_TIMEOUT)


def _check_slices(got, want, n, tag):
    covered = 0
    for r, (first, count, res) in enumerate(got):
        ref.same(res, {k: np.asarray(v)[first:first + count] for k, v in want.items()}, f"{tag} rank {r}")
        covered += count
    assert covered == n


def _cycle_case(G):
    seed = 600 + G
    nr, pr, ts, rq = cases.cluster(6000, 1501, 48, seed)
    dead = list(range(0, 6000 // G)) + list(range(6000 - 6000 // G, 6000, 3))
    return nr, pr, ts, rq, dead, seed


@pytest.mark.parametrize("G,uneven", [(2, False), (3, True), (4, False), (8, True)])
def test_nam_sharded_cycle(lb, oracle, G, uneven):
    # required sets, tombstones, a shard deleted whole, uneven shards, 1,501 pods (no multiple
    # of G), six submits (slot reuse) and more than 64 classes (two class blocks of the passes)
    nr, pr, ts, rq, dead, seed = _cycle_case(G)
    want = _want(oracle, ("cycle", G), nr, pr, ts, rq, seed, dead=dead)
    unfiltered = _want(oracle, ("cycle-unfiltered", G), nr, pr, ts, NO_REQ, seed, dead=dead)
    masks, moved = cases.coverage(want, unfiltered)
    assert masks[8] + masks[9] >= 1, masks  # a FitError whose mask has NodeAffinity's bit
    assert moved >= 1  # a SUCCESS whose winner the filter moved
    assert _classes(pr, 48) > 64
    before = lb.lb_collectives_issued()
    got = _sharded(lb, nr, pr, ts, rq, _cuts(6000, G, uneven), seed, dead=dead)
    assert lb.lb_collectives_issued() - before >= 12  # an all-gather and a reduce-scatter group per submit
    _check_slices(got, want, len(pr), f"G={G}")


def test_nam_edge_fewer_pods_than_class_keys(lb, oracle):
    # 40 pods over 48 sets: C = n_pods; 2,100 nodes: 17 row segments on one context
    nr, pr, ts, rq = cases.cluster(2100, 40, 48, 61)
    want = _want(oracle, "few-pods", nr, pr, ts, rq, 61)
    _check_slices(_sharded(lb, nr, pr, ts, rq, _cuts(2100, 3, True), 61), want, 40, "40 pods")


def test_nam_edge_empty_slices(lb, oracle):
    # 3 pods at world 8: ranks with one pod and ranks with none
    nr, pr, ts, rq = cases.cluster(300, 3, 5, 62)
    want = _want(oracle, "empty-slices", nr, pr, ts, rq, 62)
    got = _sharded(lb, nr, pr, ts, rq, _cuts(300, 8, True), 62)
    assert sorted(count for _, count, _ in got) == [0] * 5 + [1] * 3
    _check_slices(got, want, 3, "3 pods")


def test_nam_edge_rank_without_rows(lb, oracle):
    # rank 1 never upserts a node (rows_dev == 0): identity class records and key 0
    n_nodes, n_pods, n_sets, seed = cases.SHAPES[3]
    nr, pr, ts, rq = cases.cluster(n_nodes, n_pods, n_sets, seed)
    cuts = _cuts(n_nodes, 3, True)
    dead = list(range(*cuts[1]))
    want = _want(oracle, "no-rows", nr, pr, ts, rq, seed, dead=dead)
    _check_slices(_sharded(lb, nr, pr, ts, rq, cuts, seed, no_upsert=(1,)), want, n_pods, "rank 1 without rows")


def test_nam_edge_one_node_shard(lb, oracle):
    # a shard of one node (ordinal 37, alive: every 13th node is deleted, 37 is not one)
    edges = cases.SHARD_CUTS[1]
    assert edges == (0, 37, 38, 4000, 9000)
    nr, pr, ts, rq, _dead, seed = cases.shard_case(edges)
    dead = np.arange(0, 9000, 13)
    want = _want(oracle, "one-node", nr, pr, ts, rq, seed, dead=dead)
    got = _sharded(lb, nr, pr, ts, rq, list(zip(edges[:-1], edges[1:])), seed, dead=dead)
    _check_slices(got, want, len(pr), "one-node shard")


def test_nam_edge_no_tables(lb, oracle):
    # nothing registered: every pod has no terms and no requirement (two classes at most)
    n_nodes, n_pods, n_sets, seed = cases.SHAPES[3]
    nr, pr, ts, _rq = cases.cluster(n_nodes, n_pods, n_sets, seed)
    dead = np.arange(0, n_nodes, 11)
    tab = nr.copy()
    tab["allowed_pods"][dead] = -1
    want = oracle.schedule_nam_ext(tab, pr, ts[:0], literal=True, seed=seed)
    got = _sharded(lb, nr, pr, None, None, _cuts(n_nodes, 3, True), seed, dead=dead)
    _check_slices(got, {k: want[k] for k in ("node", "code", "score", "mask")}, n_pods, "no tables")


def test_nam_edge_score_weights(lb, oracle):
    weights = (7, 5)
    nr, pr, ts, rq, dead, seed = cases.weights_case(weights)
    want = _want(oracle, "weights", nr, pr, ts, rq, seed, weights=weights, dead=dead)
    got = _sharded(lb, nr, pr, ts, rq, _cuts(len(nr), 3, True), seed, dead=dead, weights=weights)
    _check_slices(got, want, len(pr), "weights (7, 5)")


@pytest.mark.parametrize("call", ["schedule_batch_batched", "schedule_batch_sequential", "schedule_sequential_device"])
def test_nam_schedule_calls_on_joined_contexts(lb, oracle, call):
    # ms_schedule_batch (both modes) and ms_schedule_sequential_device are the collective batched
    # cycle: every rank returns every pod's result, and each bind reaches its owner only
    import torch

    G, seed = 3, 63
    nr, pr, ts, rq = cases.cluster(5000, 4001, 40, seed)
    want = _want(oracle, "schedule-calls", nr, pr, ts, rq, seed)
    cuts = _cuts(5000, G, True)
    cid = _lib.comm_id_create(lb)
    dev = torch.device("cuda:0")

    def rank_fn(r):
        lo, hi = cuts[r]
        e = _engine(lb, nr, lo, hi, ts, rq, seed)
        try:
            e.comm_init(cid, r, G)
            if call == "schedule_sequential_device":
                pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
                out = torch.zeros(len(pr) * 24, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                s = torch.cuda.Stream(device=dev)
                e.schedule_sequential_device(len(pr), pods.data_ptr(), out.data_ptr(), s.cuda_stream)
                s.synchronize()
                res = out.cpu().numpy().view(_lib.RESULT).copy()
            else:
                mode = _lib.MODE_BATCHED if call == "schedule_batch_batched" else _lib.MODE_SEQUENTIAL
                res = e.schedule(pr, mode).copy()
            return res, e.read(lo, hi - lo)
        finally:
            e.close()

    got = run_ranks(G, rank_fn, timeout=RANK_TIMEOUT)
    for r, (res, _tab) in enumerate(got):
        ref.same(res, want, f"{call} rank {r}")
    cnt = np.bincount(want["node"][want["code"] == 0], minlength=len(nr))
    assert np.array_equal(np.concatenate([tab["pod_count"] for _, tab in got]), cnt)


# ---- distinct batches, slot reuse, stream modes -------------------------------------------------
SEQ_NODES, SEQ_PODS, SEQ_SETS, SEQ_SEED = 6000, 500, 48, 640
SEQ_MIX = (48, 5, 31, 48, 12, 40, 3, 48, 20, 48, 9, 36)  # term sets the pods of batch i name: 1..K
SEQ_DELTA_BEFORE, SEQ_REQ_BEFORE = 5, 9


def _seq_case(oracle):
    """Twelve different 500-pod batches, the node table before and after the delta, the required
    table before and after its replacement, and every batch's reference for what is in force at
    its submit (computed once)."""
    if "seq" in _REFS:
        return _REFS["seq"]
    nr0, _pr, ts, rq0 = cases.cluster(SEQ_NODES, SEQ_PODS, SEQ_SETS, SEQ_SEED)
    nr1 = nr0.copy()  # the delta: unschedulable and both labels change on every 7th node
    nr1["unschedulable"][::7] ^= 1
    nr1["zone"][::7] = nr1["zone"][::7] % 8 + 1
    nr1["label2"][::7] = nr1["label2"][::7] % 4 + 1
    rq1 = synth.nam_required_sets(SEQ_SETS, seed=SEQ_SEED + 1)
    batches = []
    for i, k in enumerate(SEQ_MIX):
        p = synth.pods(SEQ_PODS, seed=SEQ_SEED + 1 + i, start=SEQ_PODS * i, term_sets=k)
        p["name_digit"][::23] = -1
        p["tolerates_unschedulable"][::9] = 1
        batches.append(p)

    def run(i, nr, rq):
        return ref.schedule_tombstone(oracle, nr, batches[i], ts, rq, seed=SEQ_SEED)

    want = [run(i, nr1 if i >= SEQ_DELTA_BEFORE else nr0, rq1 if i >= SEQ_REQ_BEFORE else rq0)
            for i in range(len(batches))]

    def differ(a, b):
        return any(not np.array_equal(a[k], b[k]) for k in ("node", "code", "score", "mask"))

    # a stale table must be visible in the first batch after each change
    assert differ(run(SEQ_DELTA_BEFORE, nr0, rq0), want[SEQ_DELTA_BEFORE])
    assert differ(run(SEQ_REQ_BEFORE, nr1, rq0), want[SEQ_REQ_BEFORE])
    for i in range(1, len(batches)):
        assert differ(want[i - 1], want[i])
    _REFS["seq"] = (nr0, nr1, ts, rq0, rq1, batches, want)
    return _REFS["seq"]


@pytest.mark.parametrize("mode", ["one_caller_stream", "alternating_caller_streams", "two_sweep_streams"])
def test_nam_distinct_batches_slot_reuse(lb, oracle, monkeypatch, mode):
    # twelve submits at world 2 (two rounds of slot reuse at depth 4), each a DIFFERENT batch into
    # its own result buffer, a node delta before submit 5, the required table replaced before
    # submit 9, no host synchronise of the caller streams before the final drains. The context's
    # one NodeAffinity scratch passes from batch to batch (nam_take / nam_release): a keys pass
    # that resumed from another batch's class pass, or a fence that followed the segment pass but
    # not the keys pass, gives some batch another batch's or another table's result
    import torch

    if mode == "two_sweep_streams":
        monkeypatch.setenv("MINISCHED_SHARD_STREAMS", "2")
    nr0, nr1, ts, rq0, rq1, batches, want = _seq_case(oracle)
    G = 2
    cuts = _cuts(SEQ_NODES, G)
    cid = _lib.comm_id_create(lb)
    dev = torch.device("cuda:0")

    def rank_fn(r):
        lo, hi = cuts[r]
        e = _engine(lb, nr0, lo, hi, ts, rq0, SEQ_SEED)
        try:
            e.comm_init(cid, r, G)
            slices = [e.sharded_slice(len(p)) for p in batches]
            pods = [torch.from_numpy(p.view(np.uint8).copy()).to(dev) for p in batches]
            res = [torch.full((max(1, count) * 24,), 0xAB, dtype=torch.uint8, device=dev) for _, count in slices]
            torch.cuda.synchronize()
            ss = [torch.cuda.Stream(device=dev) for _ in range(2)]
            for i in range(len(batches)):
                if i == SEQ_DELTA_BEFORE:
                    e.upsert(np.arange(lo, hi), nr1[lo:hi])
                    e.flush()
                if i == SEQ_REQ_BEFORE:
                    e.nam_required_sets(rq1)
                s = ss[i % 2] if mode == "alternating_caller_streams" else ss[0]
                e.sharded_submit(len(batches[i]), pods[i].data_ptr(), res[i].data_ptr(), s.cuda_stream)
            for s in ss:
                e.sharded_drain(s.cuda_stream)
            torch.cuda.synchronize()
            return [(first, count, x.cpu().numpy().view(_lib.RESULT)[:count].copy())
                    for (first, count), x in zip(slices, res)]
        finally:
            e.close()

    got = run_ranks(G, rank_fn, timeout=RANK_TIMEOUT)
    for i in range(len(batches)):
        _check_slices([got[r][i] for r in range(G)], want[i], len(batches[i]), f"{mode} batch {i}")


def test_nam_class_form_equals_caller_collective_form(lb, oracle):
    # the pod-record form a caller with its own collectives drives (ms_nam_segment_device ->
    # gather -> ms_nam_keys_device -> uint64 MAX, ms_nam_flags_device, ms_decode_device) on
    # unjoined contexts of the same shards, against the in-library class-record form: the same
    # function, element for element, and both the reference's
    import torch

    G = 4
    nr, pr, ts, rq, dead, seed = _cycle_case(G)
    want = _want(oracle, ("cycle", G), nr, pr, ts, rq, seed, dead=dead)
    cuts = _cuts(6000, G, False)
    got = _sharded(lb, nr, pr, ts, rq, cuts, seed, dead=dead, steps=1)
    inlib = np.concatenate([res for _, _, res in got])
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    P, SB = len(pr), _lib.NAM_SEG_BYTES
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    segs = torch.zeros(G * P * SB, dtype=torch.uint8, device=dev)
    keys = torch.zeros((G, P), dtype=torch.int64, device=dev)
    flags = torch.full((P,), -1, dtype=torch.int32, device=dev)
    out = torch.zeros(P * 24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engines = [_engine(lb, nr, lo, hi, ts, rq, seed, dead) for lo, hi in cuts]
    try:
        for g, e in enumerate(engines):
            e.nam_segment_device(P, pods.data_ptr(), segs.data_ptr() + g * P * SB, s.cuda_stream)
        for g, e in enumerate(engines):
            e.nam_keys_device(P, pods.data_ptr(), G, g, segs.data_ptr(), keys[g].data_ptr(), s.cuda_stream)
        engines[-1].nam_flags_device(P, G, segs.data_ptr(), flags.data_ptr(), s.cuda_stream)
        s.synchronize()
        best = keys.max(dim=0).values.contiguous()  # keys < 2^63: the signed max is the unsigned one
        present = sum(int(e.info().present_nodes) for e in engines)
        torch.cuda.synchronize()
        engines[0].decode_device(P, pods.data_ptr(), best.data_ptr(), flags.data_ptr(), present, out.data_ptr(),
                                 s.cuda_stream)
        s.synchronize()
        hand = out.cpu().numpy().view(_lib.RESULT).copy()
    finally:
        for e in engines:
            e.close()
    ref.same(hand, want, "caller-collective form")
    ref.same(inlib, want, "in-library form")
    for k in ("node", "code", "score", "plugin_mask"):
        assert np.array_equal(hand[k], inlib[k]), k
