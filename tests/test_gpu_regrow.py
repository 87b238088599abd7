"""Scratch that grows inside a live context, and contexts that give their memory back.

Every grow-on-demand routine of the host layer (mini-kube-scheduler_amd/csrc/ms_capi.cpp,
ms_cycle.cpp, ms_seq_host.cpp, ms_hostarray.cpp, ms_comm.cpp; DESIGN.md "Who frees what") releases the buffers it held and allocates larger
ones. Each case here takes ONE context, makes a call, then a larger call that forces the
routine to grow, and compares both results bit for bit with the CPU oracle: a buffer
released while still in use, a stale capacity or a view left pointing into a released
block shows up as a wrong result. test_context_cycles_return_memory then opens and closes
contexts in a loop and watches the device's free memory. The sharp test of the owner type
itself is on the CPU (tests/cpp/test_owned.cpp).
"""
import numpy as np
import pytest

import test_gpu_loopback as lbk
import test_gpu_nam as nam
import test_gpu_taint as tt
from minisched_amd import _lib, synth
from test_gpu_loopback import lb  # noqa: F401  (the loopback library fixture)

pytestmark = pytest.mark.gpu

NRF, NA = _lib.PLUGINS_NU_NRF_NN_LA, _lib.PLUGINS_NU_NN_NA
FIELDS = (("node", "node"), ("code", "code"), ("score", "score"), ("plugin_mask", "mask"))
BOUND = ("pod_count", "req_cpu", "req_mem", "nz_cpu", "nz_mem")  # the oracle's columns a bind changes


def _same(res, o, tag, a=0, b=None):
    tt._same(res, o, tag, a, b)


def _commit(cols, o, pr):
    # MS_MODE_BATCHED on the resource-aware set: every pod decided on one state, then the binds
    for j in np.nonzero(o["code"] == 0)[0]:
        i = int(o["node"][j])
        cols.pod_count[i] += 1
        cols.req_cpu[i] += pr["req_milli_cpu"][j]
        cols.req_mem[i] += pr["req_memory"][j]
        cols.nz_cpu[i] += pr["nonzero_milli_cpu"][j]
        cols.nz_mem[i] += pr["nonzero_memory"][j]


def _table_same(e, cols, n, tag):
    t = e.read(0, n)
    for k_dev, k_or in (("pod_count", "pod_count"), ("req_milli_cpu", "req_cpu"), ("req_memory", "req_mem"),
                        ("nonzero_milli_cpu", "nz_cpu"), ("nonzero_memory", "nz_mem")):
        assert np.array_equal(t[k_dev], getattr(cols, k_or)[:n]), f"{tag}: column {k_dev}"


# ---- the resource-aware context of the stage and tile cases -----------------------------
R_SEED, R_NODES, R_SMALL = 61, 1500, 300


def _nrf_cluster():
    nr = synth.nodes(R_NODES, seed=R_SEED, resources=True)
    pr = synth.pods(1400, seed=R_SEED, resources=True)
    pr["name_digit"][::23] = -1
    pr["tolerates_unschedulable"][::9] = 1
    return nr, pr


def _nrf_engine(nr):
    e = _lib.Engine(max_nodes=R_NODES, plugin_set=NRF, seed=R_SEED, max_batch=256)
    e.upsert(np.arange(R_SMALL), nr[:R_SMALL])
    return e


def _stage_calls(e, pr):
    # ensure_stage: a batched call on this set is ONE pass over all its pods, so 700 pods
    # outgrow the staging of max_batch = 256 that 200 pods fit
    return e.schedule(pr[:200], _lib.MODE_BATCHED), e.schedule(pr[200:900], _lib.MODE_BATCHED)


def _tile_calls(e, nr, pr, a=900):
    # ensure_tiles: 300 rows are 5 sweep tiles, 1,500 rows 24
    r1 = e.schedule(pr[a:a + 250], _lib.MODE_SEQUENTIAL)
    e.upsert(np.arange(R_SMALL, R_NODES), nr[R_SMALL:])
    return r1, e.schedule(pr[a + 250:a + 500], _lib.MODE_SEQUENTIAL)


def test_regrow_stage(oracle):
    nr, pr = _nrf_cluster()
    cols = oracle.NodeCols(nr[:R_SMALL])
    with _nrf_engine(nr) as e:
        r1, r2 = _stage_calls(e, pr)
        for r, p, tag in ((r1, pr[:200], "200 pods"), (r2, pr[200:900], "700 pods")):
            o = oracle.schedule(nr[:R_SMALL], p, plugin_set=1, mode=0, seed=R_SEED, cols=cols)
            _same(r, o, tag)
            _commit(cols, o, p)
        _table_same(e, cols, R_SMALL, "after both calls")
    assert cols.pod_count.sum() > 450  # (most of the 900 pods were placed, so the second call saw the first's binds)


def test_regrow_tiles(oracle):
    nr, pr = _nrf_cluster()
    with _nrf_engine(nr) as e:
        r1, r2 = _tile_calls(e, nr, pr, a=0)
        small = oracle.NodeCols(nr[:R_SMALL])
        _same(r1, oracle.schedule(nr[:R_SMALL], pr[:250], plugin_set=1, mode=1, seed=R_SEED, cols=small), "300 nodes")
        cols = oracle.NodeCols(nr)  # the first call's binds stay on the first 300 rows
        for k in BOUND:
            getattr(cols, k)[:R_SMALL] = getattr(small, k)
        o2 = oracle.schedule(nr, pr[250:500], plugin_set=1, mode=1, seed=R_SEED, cols=cols)
        _same(r2, o2, "1500 nodes")
        _table_same(e, cols, R_NODES, "after both calls")
        assert e.info()._pad == 0
    assert (o2["node"][o2["code"] == 0] >= R_SMALL).any()


# ---- compact records --------------------------------------------------------------------
def _compact_same(r, o, tag, a, b):
    for k_res, k_or in FIELDS:
        got, want = r[k_res].astype(np.int64), o[k_or][a:b].astype(np.int64)
        assert np.array_equal(got, want), f"{tag}: {k_res} differs at {np.nonzero(got != want)[0][:8].tolist()}"


def _compact_calls(e, pr):
    c = _lib.compact_pods(pr)
    return e.schedule_compact(c[:300]), e.schedule_compact(c[300:1500])


def test_regrow_zero_copy_staging(oracle):
    # ensure_zc: the pinned records of the single-shard NU+NN compact cycle, 300 then 1,200 pods
    seed = 62
    nr, pr = synth.nodes(300, seed=seed), synth.pods(1500, seed=seed)
    pr["name_digit"][::13] = -1
    pr["tolerates_unschedulable"][::6] = 1
    o = oracle.schedule(nr, pr, seed=seed)  # (stateless: no pod's outcome depends on another's)
    with _lib.Engine(max_nodes=300, seed=seed) as e:
        e.upsert(np.arange(300), nr)
        r1, r2 = _compact_calls(e, pr)
        _compact_same(r1, o, "300 pods", 0, 300)
        _compact_same(r2, o, "1200 pods", 300, 1500)
        placed = np.bincount(o["node"][o["code"] == 0], minlength=300)
        assert np.array_equal(e.read(0, 300)["pod_count"], placed)


def _na_engine(nr, seed):
    e = _lib.Engine(max_nodes=len(nr), plugin_set=NA, seed=seed, max_batch=256)
    e.upsert(np.arange(len(nr)), nr)
    return e


def test_regrow_compact_staging(oracle):
    # the staged compact cycle (NU+NN+NA): d_podc / d_resc from nothing to 300 to 1,200
    # records, and ensure_stage from max_batch = 256 to 300 to 1,200 pods
    seed = 63
    nr, pr = synth.nodes(300, seed=seed, zones=True), synth.pods(1500, seed=seed, zones=True)
    pr["name_digit"][::17] = -1
    pr["tolerates_unschedulable"][::6] = 1
    o = oracle.schedule_na(nr, pr, literal=True, seed=seed)
    with _na_engine(nr, seed) as e:
        r1, r2 = _compact_calls(e, pr)
        _compact_same(r1, o, "300 pods", 0, 300)
        _compact_same(r2, o, "1200 pods", 300, 1500)
    assert len(np.unique(o["score"])) > 4


# ---- TaintToleration, multi-term NodeAffinity, node deltas ------------------------------
def test_regrow_tt_scratch(oracle):
    # ensure_tt: the two-pass cycle's scratch for chunks of 100, then of 256 pods
    seed = 64
    nr, pr, dead = tt._cluster(300, 256, seed, dead_every=11)
    o = tt._oracle(oracle, nr, pr, seed, dead, literal=True)
    with tt._engine(nr, seed, dead=dead, max_batch=256) as e:
        _same(e.schedule(pr[:100]), o, "100 pods", 0, 100)
        _same(e.schedule(pr), o, "256 pods")
    assert (o["code"] == 0).sum() > 100


def test_regrow_nam_term_table(oracle):
    # nam_install: 3 term sets, a cycle, 40 term sets (a larger table), a cycle
    seed = 65
    nr, pr3, ts3 = nam._cluster(300, 200, 3, seed)
    _, pr40, ts40 = nam._cluster(300, 200, 40, seed)
    with nam._engine(nr, ts3, seed) as e:
        _same(e.schedule(pr3), nam._oracle(oracle, nr, pr3, ts3, seed), "3 term sets")
        e.nam_term_sets(ts40)
        _same(e.schedule(pr40), nam._oracle(oracle, nr, pr40, ts40, seed), "40 term sets")
    assert len(np.unique(pr40["pref_zone"])) > 20


def _delta_records(n, seed):
    rec = synth.nodes(n, seed=seed, resources=True, labels=True, taints=True)
    rng = np.random.default_rng(seed)
    rec["pod_count"] = rng.integers(0, 100, n)
    for f in ("req_milli_cpu", "req_memory", "nonzero_milli_cpu", "nonzero_memory"):
        rec[f] = rng.integers(0, 1 << 40, n)
    return rec


def test_regrow_delta_staging():
    # ensure_delta_cap: 100 rows (staging for 1,024), then 3,000 rows; the records read back
    # are the ones upserted, field by field
    with _lib.Engine(max_nodes=3000, plugin_set=NRF, seed=66) as e:
        for n, seed in ((100, 66), (3000, 67)):
            rec = _delta_records(n, seed)
            e.upsert(np.arange(n), rec)
            e.flush()
            got = e.read(0, n)
            for f in _lib.NODE_REC.names:
                assert np.array_equal(got[f], rec[f]), f"{n} rows: field {f}"
        assert e.info().present_nodes == 3000


# ---- the combine buffers of a communicator's slots --------------------------------------
def test_regrow_shard_slots(lb, oracle):  # noqa: F811
    # slot_ensure at world 2 (the loopback build): slices of 250 pods fit the slots' 1,024;
    # slices of 1,500 do not. 6 submits each, so every one of the 5 slots is used at the
    # small size and then grown
    import torch

    G, seed, n = 2, 68, 600
    nr, pr = synth.nodes(n, seed=seed), synth.pods(3500, seed=seed)
    pr["name_digit"][::17] = -1
    o = oracle.schedule(nr, pr, seed=seed)  # (stateless: the two batches are slices of one run)
    cuts = lbk._cuts(n, G)
    cid = _lib.comm_id_create(lb)
    dev = torch.device("cuda:0")
    batches = ((0, 500), (500, 3500))

    def rank_fn(r):
        e = lbk._joined(lb, cid, r, G, nr, cuts[r][0], cuts[r][1], _lib.PLUGINS_NU_NN, seed)
        try:
            out = []
            s = torch.cuda.Stream(device=dev)
            for a, b in batches:
                first, count = e.sharded_slice(b - a)
                pods = torch.from_numpy(pr[a:b].view(np.uint8).copy()).to(dev)
                res = torch.full((max(1, count) * 24,), 0xAB, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()  # (the copy and the fill ran on torch's stream, not s)
                for _ in range(6):
                    e.sharded_submit(b - a, pods.data_ptr(), res.data_ptr(), s.cuda_stream)
                e.sharded_drain(s.cuda_stream)
                s.synchronize()
                out.append((first, count, res.cpu().numpy().view(_lib.RESULT)[:count].copy()))
            return out
        finally:
            e.close()

    got = lbk.run_ranks(G, rank_fn, timeout=120)
    for (a, b), k in zip(batches, range(2)):
        assert sum(got[r][k][1] for r in range(G)) == b - a
        for r in range(G):
            first, count, res = got[r][k]
            lbk._same(res, o, a + first, a + first + count, f"{b - a} pods, rank {r}")


# ---- contexts give their memory back ----------------------------------------------------
def _cycle(inputs, before_close=None):
    # host-array calls only: no torch tensor is allocated in here. The resource-aware context
    # runs the stage and tile calls above; the compact entry point refuses that plugin set, so
    # the compact calls (zero-copy, and staged) run on an NU+NN and an NU+NN+NA context
    nr, pr, nr0, pr0, nr2, pr2 = inputs
    ctxs = [_nrf_engine(nr), _lib.Engine(max_nodes=300, seed=62), _na_engine(nr2, 63)]
    try:
        _stage_calls(ctxs[0], pr)
        _tile_calls(ctxs[0], nr, pr)
        ctxs[1].upsert(np.arange(300), nr0)
        _compact_calls(ctxs[1], pr0)
        _compact_calls(ctxs[2], pr2)
        return before_close() if before_close else None
    finally:
        for e in ctxs:
            e.close()


def test_context_cycles_return_memory():
    """F0 - F2 < (F0 - F1) / 4, with F0 the device's free memory after a warm-up cycle, F1
    with one cycle's contexts open and used, F2 after 12 more cycles: a buffer group of at
    least 1/48 of a cycle's footprint that leaks every cycle trips it. It cannot see a leak
    below the runtime's allocation granule (the CPU test is the sharp one)."""
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    inputs = _nrf_cluster() + (synth.nodes(300, seed=62), synth.pods(1500, seed=62),
                               synth.nodes(300, seed=63, zones=True), synth.pods(1500, seed=63, zones=True))
    _cycle(inputs)  # warm-up: code objects, the runtime's own pools
    f0 = free()
    f1 = _cycle(inputs, before_close=free)
    for _ in range(12):
        _cycle(inputs)
    f2 = free()
    print(f"free device memory: F0 - F1 = {f0 - f1} B (one cycle's contexts), F0 - F2 = {f0 - f2} B after 13 cycles")
    assert f0 - f1 > 0, "the open contexts hold no device memory?"
    assert f0 - f2 < (f0 - f1) / 4
