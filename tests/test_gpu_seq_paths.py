"""The sequential validator's routes (ms_seq.hip: validate_batch, walk_top4,
validate_scan, the prologue's stale re-resolution, merge_pod_lists' certified
ranks), each reached on purpose by the directed contention cases of
tests/_seq_path_cases.py and pinned by the counters of ms_seq_counters.

The parity tests draw random clusters; which route decides a pod follows from the
draw. Here a few hot rows are feasible and a whole batch contends for them, so
tests/test_seq_path_cases.py can prove on the CPU which routes run, and this
module asserts on the GPU that they did: results, masks and tables against the C
oracle, and the counter deltas of the call against simulate_batch, the
validator's rounds restated in Python integers. Every batch of a plateau case
has a known stale set (the filler pods bind nothing; a (pod, row) key does not
move on the plateau), so the expected counters are exact and asserted with ==.

The structural classes of classify() (rows bound by EARLIER PODS of the batch)
are NOT lower bounds on the counters of this design: a pod is resolved against
the state at the start of its round and decided in that round when no earlier
undecided pod claims its winner, so it does not see the binds of the pods between
the round's start and itself (case spread8: 33 structural scans, 27 by the
rounds, on the CPU and on the GPU). The lower bounds asserted here are therefore
the restated rounds' own counts.
"""
import numpy as np
import pytest

import _seq_path_cases as sp
from minisched_amd import _lib
from minisched_amd._lib import MODE_SEQUENTIAL, NODE_REC, PLUGINS_NU_NRF_NN_LA, POD_REC, RESULT, SEQ_CAND, SEQ_TOPK, Engine

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in sp.CASES]
BIND_COLS = (("pod_count", "pod_count"), ("req_milli_cpu", "req_cpu"), ("req_memory", "req_mem"),
             ("nonzero_milli_cpu", "nz_cpu"), ("nonzero_memory", "nz_mem"))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    _lib.load()
    if _lib.device_count() == 0:
        pytest.fail("gpu test collected on a host without a visible device")


@pytest.fixture(scope="module")
def tile_rows():
    import torch

    return sp.tile_rows_for(sp.N_NODES, torch.cuda.get_device_properties(0).multi_processor_count)


def same(res, o, a, b, tag):
    for k_res, k_or in (("node", "node"), ("code", "code"), ("score", "score"), ("plugin_mask", "mask")):
        got, want = res[k_res], o[k_or][a:b]
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{tag} {k_res}: pod {a + bad[0]} gpu {got[bad[0]]} oracle {want[bad[0]]} ({len(bad)} differ)"
    assert not res["_pad"].any()


def load(e, nodes, gone, lo=0, hi=sp.N_NODES):
    e.upsert(np.arange(lo, hi), nodes[lo:hi])
    g = gone[(gone >= lo) & (gone < hi)]
    if len(g):
        e.delete(g.astype(np.uint32))
    e.flush()


def counters(e):
    c = e.seq_counters()
    return {k: getattr(c, k) for k in ("overflow", "resweep_tiles", "recomputes", "pods", "misses", "slow_pods",
                                       "list_scans")}


@pytest.mark.parametrize("merge", [None, "launch", "fallback"])
@pytest.mark.parametrize("name", NAMES)
def test_routes_single_context(oracle, monkeypatch, tile_rows, name, merge):
    if merge is not None:
        monkeypatch.setenv("MINISCHED_SEQ_MERGE", merge)
    case = sp.CASE[name]
    nodes, gone, pods, n_fill, o = sp.prepared(case, oracle, NODE_REC, POD_REC, tile_rows)
    with Engine(max_nodes=sp.N_NODES, plugin_set=PLUGINS_NU_NRF_NN_LA, seed=sp.SEED) as e:
        load(e, nodes, gone)
        before = counters(e)
        res = e.schedule(pods, MODE_SEQUENTIAL)
        after = counters(e)
        back = e.read(0, sp.N_NODES)
        info = e.info()
    d = {k: after[k] - before[k] for k in after}
    cls, sim = sp.run_model(case, nodes, pods, o, tile_rows, simulate=case.bounds)
    print(f"{name}[{merge}] tile_rows {tile_rows}: gpu {d} rounds' model {dict(sim)} structural {dict(cls)}")
    same(res, o, 0, len(pods), f"{name}[{merge}]")
    for k_dev, k_or in BIND_COLS:
        assert np.array_equal(back[k_dev], getattr(o["cols"], k_or)), k_dev
    assert after["overflow"] == 0 and info._pad == 0
    # ms_info carries three of the counters
    assert (info.seq_pods, info.seq_resweep_tiles, info.seq_recomputes) == (after["pods"], after["resweep_tiles"],
                                                                          after["recomputes"])
    assert d["pods"] == len(pods)
    if case.bounds:
        # every batch's stale set is known (module docstring): the rounds' counts, exactly
        assert d["list_scans"] == sim["scan"]
        assert d["slow_pods"] == sim["slow"]
        assert d["resweep_tiles"] == sim["resweep"]
        assert d["recomputes"] == sim["recompute"]
        for w in case.want:  # and the route the case is named for did run
            if w in ("scan", "resweep"):
                assert d[{"scan": "list_scans", "resweep": "resweep_tiles"}[w]] >= 1


def _shard_cuts(G):
    # uneven shards whose borders fall inside tiles, not on 16-row blocks
    return [0] + [sp.N_NODES * g // G + 7 * g for g in range(1, G)] + [sp.N_NODES]


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("name", NAMES)
def test_routes_node_sharded_contexts(oracle, tile_rows, name, G):
    # ms_seq_candidates_device / ms_seq_validate_device over G contexts on one GPU (the
    # all-gather by concatenation): a window ends before a pod that the gathered
    # candidates cannot decide, so the one-block cases advance in many short windows;
    # every pod is decided in the end, as the oracle decides it
    import torch

    case = sp.CASE[name]
    nodes, gone, pods, n_fill, o = sp.prepared(case, oracle, NODE_REC, POD_REC, tile_rows)
    pr, n = pods[n_fill:], case.n  # (the filler only sizes the single context's batches)
    assert (o["code"][:n_fill] != sp.CODE_SUCCESS).all()
    cuts, batch = _shard_cuts(G), 64
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    sp_ = s.cuda_stream
    dpods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    engines = []
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            e = Engine(max_nodes=b - a, plugin_set=PLUGINS_NU_NRF_NN_LA, node_base=a, seed=sp.SEED)
            engines.append(e)
            load(e, nodes, gone, a, b)
        cb = SEQ_CAND.itemsize * SEQ_TOPK
        cands = [torch.zeros(batch * cb, dtype=torch.uint8, device=dev) for _ in range(G)]
        flags = [torch.zeros(batch, dtype=torch.int32, device=dev) for _ in range(G)]
        res = [torch.zeros(n * 24, dtype=torch.uint8, device=dev) for _ in range(G)]
        done = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(G)]
        a, windows = 0, 0
        while a < n:
            nb = min(batch, n - a)
            for g, e in enumerate(engines):
                e.seq_candidates_device(nb, dpods.data_ptr() + 40 * a, cands[g].data_ptr(), flags[g].data_ptr(), sp_)
            with torch.cuda.stream(s):
                call = torch.cat([c[: nb * cb] for c in cands])
                fall = torch.cat([f[:nb] for f in flags])
            for g, e in enumerate(engines):
                e.seq_validate_device(nb, dpods.data_ptr() + 40 * a, G, call.data_ptr(), fall.data_ptr(),
                                      res[g].data_ptr() + 24 * a, done[g].data_ptr(), sp_)
            s.synchronize()
            nd = [int(x.item()) for x in done]
            assert len(set(nd)) == 1 and 1 <= nd[0] <= nb, nd  # every window decides its first pod at least
            a += nd[0]
            windows += 1
            assert windows <= n
        assert a == n
        tables = [e.read(lo, hi - lo) for e, lo, hi in zip(engines, cuts[:-1], cuts[1:])]
    finally:
        for e in engines:
            e.close()
    for g in range(G):
        same(res[g].cpu().numpy().view(RESULT), o, n_fill, n_fill + n, f"{name} shard {g}/{G}")
    t = np.concatenate(tables)
    for k_dev, k_or in BIND_COLS:
        assert np.array_equal(t[k_dev], getattr(o["cols"], k_or)), k_dev


@pytest.mark.parametrize("window", ["7", "128"])
def test_routes_library_device_cursor(oracle, monkeypatch, tile_rows, window):
    # ms_schedule_sequential_device on a 1-rank communicator, the queue cursor on the
    # device: the directed pods of one case per kind, one context per case
    import torch

    from minisched_amd import sharded

    monkeypatch.setenv("MINISCHED_SHARD_SEQ_BATCH", window)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    for name in ("block6_hi", "two_blocks5", "block6_room3_masks"):
        case = sp.CASE[name]
        nodes, gone, pods, n_fill, o = sp.prepared(case, oracle, NODE_REC, POD_REC, tile_rows)
        pr = pods[n_fill:]
        e = Engine(max_nodes=sp.N_NODES, plugin_set=PLUGINS_NU_NRF_NN_LA, seed=sp.SEED)
        try:
            load(e, nodes, gone)
            sharded.init_comm(e)
            dpods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
            seq = sharded.ShardedSequential(e, len(pr), dpods, stream)
            assert seq.library
            res = seq.run()
            stream.synchronize()
            res = res.cpu().numpy().view(RESULT)
            back = e.read(0, sp.N_NODES)
        finally:
            e.close()
        same(res, o, n_fill, len(pods), f"{case.name} window {window}")
        for k_dev, k_or in BIND_COLS:
            assert np.array_equal(back[k_dev], getattr(o["cols"], k_or)), (case.name, k_dev)
