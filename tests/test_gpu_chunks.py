"""Chunk boundaries: calls of more than max_batch pods, which every device entry
point cuts into chunks of max_batch pods itself. Each test hands the library
ALL its pods in one call and compares node, code, score and plugin_mask bit for
bit with the CPU oracle; the host-array tests also compare the bind counts in
the table.

The multi-term NodeAffinity (NAM) shapes are the ones where a layout of the
short last chunk's own pod count needs more scratch than the allocation sized
for the full chunk holds (mini-kube-scheduler_amd/csrc/ms_nam_layout.h):
tests/cpp/test_nam_layout.cpp shows on the CPU, for exactly these shapes, that
the rule the library had before overran the shard inputs by more than 64 KiB,
and that the plan it uses now keeps every chunk inside. Every pod of a chunk
there is a class of its own, so the per-class arrays are used to their end.

Oracle forms. NAM: the literal O(F^2) loop, run on slices of the pods in
threads, for every case of up to 3000 nodes; its closed form (tied to the loop
in tests/test_oracle_nam.py) for the one three-shard case of 3300 nodes, whose
shards cannot be smaller: at 255 term sets and max_batch 512 only row counts
of 1025 to about 1200 overran. TaintToleration: the literal loop. NU+NN+NA:
the literal loop at 300 nodes, the closed form at 5000. NU+NN: the OpenMP
oracle.
"""
import numpy as np
import pytest

import test_gpu_nam as nam
import test_gpu_taint as tt
from minisched_amd import _lib, synth
from minisched_amd.hostinfo import cpu_threads

pytestmark = pytest.mark.gpu

_CACHE = {}


def _once(key, make):
    # inputs and oracle results are computed once and shared; no test writes to them
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _by_pod_slices(run, pr):
    # the literal loops are single-threaded and O(F^2) per pod; these plugin sets read no state a
    # bind changes, so a pod's outcome depends on the nodes and its own record only: the same
    # oracle call on slices of the pods, in threads (ctypes drops the GIL), joined in pod order
    from concurrent.futures import ThreadPoolExecutor

    k = max(1, min(cpu_threads(), 16, len(pr) // 32))
    cuts = [len(pr) * i // k for i in range(k + 1)]
    with ThreadPoolExecutor(k) as ex:
        parts = list(ex.map(lambda ab: run(pr[ab[0]:ab[1]]), zip(cuts[:-1], cuts[1:])))
    return {f: np.concatenate([p[f] for p in parts]) for f in ("node", "code", "score", "mask")}


def _same(res, o, tag, a=0, b=None):
    tt._same(res, o, tag, a, b)


def _device_cycle(e, pr):
    return nam._device_cycle(e, pr)


# ---- multi-term NodeAffinity ------------------------------------------------------------
# rows on a context, term sets, max_batch, pods (tests/cpp/test_nam_layout.cpp: kGpuShapes)
NAM_SHAPES = {"576x1984": (576, 511, 1024, 1984), "1100x960": (1100, 255, 512, 960)}


def _nam_inputs(shape, n_nodes, ext, seed):
    def make():
        _, n_sets, max_batch, n_pods = NAM_SHAPES[shape]
        nr, pr, ts = (nam._ext_cluster if ext else nam._cluster)(n_nodes, n_pods, n_sets, seed)
        j = np.arange(n_pods)
        sid = (j * 7919) % (n_sets + 1)
        pr["pref_zone"], pr["pref_weight"] = sid & 0xFF, sid >> 8
        pr["tolerates_unschedulable"] = (j // (n_sets + 1)) & 1
        # n_sets + 1 is a power of two and 7919 is odd: every chunk holds as many classes as pods
        assert (n_sets + 1) & n_sets == 0 and n_pods > max_batch and n_pods % max_batch
        key = (pr["pref_zone"].astype(np.int64) | pr["pref_weight"].astype(np.int64) << 8) * 2 \
            + pr["tolerates_unschedulable"]
        for s0 in range(0, n_pods, max_batch):
            assert len(np.unique(key[s0:s0 + max_batch])) == min(max_batch, n_pods - s0)
        assert (pr["name_digit"] < 0).any()
        return nr, pr, ts
    return _once(("nam-in", shape, n_nodes, ext, seed), make)


def _nam_oracle(oracle, tag, nr, pr, ts, seed, weights, dead, literal):
    def make():
        x = nr.copy()
        if len(dead):
            x["allowed_pods"][np.asarray(dead)] = -1
        run = oracle.schedule_nam_ext if nam._ext(ts) else oracle.schedule_nam
        return _by_pod_slices(lambda p: run(x, p, ts, weights=weights, literal=literal, seed=seed), pr)
    return _once(("nam-or", tag, len(nr), len(pr), nam._ext(ts), seed, weights, literal), make)


def _one_context_seed(rows, ext):
    return 80 + rows % 7 + (1 if ext else 0)


@pytest.mark.parametrize("shape,ext,weights", [("576x1984", False, (1, 1)), ("576x1984", True, (3, 2)),
                                               ("1100x960", False, (1, 1)), ("1100x960", True, (1, 1))])
def test_nam_short_last_chunk(oracle, shape, ext, weights):
    # ms_select_batch_device on one context: chunks 1024 + 960 and 512 + 448
    rows, _, max_batch, _ = NAM_SHAPES[shape]
    seed = _one_context_seed(rows, ext)
    nr, pr, ts = _nam_inputs(shape, rows, ext, seed)
    dead = np.arange(0, rows, 7)
    o = _nam_oracle(oracle, "every 7th dead", nr, pr, ts, seed, weights, dead, literal=True)
    with nam._engine(nr, ts, seed, dead=dead, weights=weights, max_batch=max_batch) as e:
        _same(_device_cycle(e, pr), o, f"{shape} ext {ext}")
    assert (o["code"] == 0).sum() > 0.8 * len(pr) and len(np.unique(o["score"])) > 4


@pytest.mark.parametrize("shape,cuts,ext,middle_dead", [
    ("576x1984", (0, 576, 1152), False, False), ("576x1984", (0, 576, 1152, 1728), True, False),
    ("1100x960", (0, 1100, 2200), True, False), ("1100x960", (0, 1100, 2200, 3300), False, False),
    ("576x1984", (0, 576, 1152, 1728), False, True)])
def test_nam_short_last_chunk_node_shards(oracle, shape, cuts, ext, middle_dead):
    # ms_nam_segment_device -> ms_nam_keys_device -> uint64 MAX -> ms_decode_device, every shard
    # with a row count at which the last chunk's own layout overran; in ms_nam_keys_device the
    # overrun landed on the rescale records just composed for the chunk
    import torch

    _, _, max_batch, _ = NAM_SHAPES[shape]
    seed = 90 + len(cuts) + (1 if ext else 0)
    n = cuts[-1]
    nr, pr, ts = _nam_inputs(shape, n, ext, seed)
    dead = np.arange(cuts[1], cuts[2]) if middle_dead else np.arange(0, n, 13)
    o = _nam_oracle(oracle, "middle dead" if middle_dead else "every 13th dead", nr, pr, ts, seed, (1, 1), dead,
                    literal=n <= 3000)  # (the module docstring: which form where)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    G, P, SB = len(cuts) - 1, len(pr), _lib.NAM_SEG_BYTES
    segs = torch.zeros(G * P * SB, dtype=torch.uint8, device=dev)
    keys = torch.zeros((G, P), dtype=torch.int64, device=dev)
    out = torch.full((P * 24,), 0xCD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (the fills ran on torch's stream, not s)
    engines = [nam._engine(nr, ts, seed, lo, hi, dead, max_batch=max_batch) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        for g, e in enumerate(engines):
            e.nam_segment_device(P, pods.data_ptr(), segs.data_ptr() + g * P * SB, s.cuda_stream)
        for g, e in enumerate(engines):
            e.nam_keys_device(P, pods.data_ptr(), G, g, segs.data_ptr(), keys[g].data_ptr(), s.cuda_stream)
        s.synchronize()
        best = keys.max(dim=0).values.contiguous()  # keys < 2^63: the signed max is the unsigned one
        present = sum(int(e.info().present_nodes) for e in engines)
        torch.cuda.synchronize()
        engines[0].decode_device(P, pods.data_ptr(), best.data_ptr(), 0, present, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        _same(out.cpu().numpy().view(_lib.RESULT), o, f"{shape} shards {cuts}")
    finally:
        for e in engines:
            e.close()
    if middle_dead:
        won = o["node"][o["code"] == 0]
        assert ((won < cuts[1]) | (won >= cuts[2])).all() and (won < cuts[1]).any() and (won >= cuts[2]).any()


def test_nam_scratch_reuse_across_chunkings(oracle):
    # one engine: a one-chunk call, a call of 1024 + 960 pods, the one-chunk call again (scratch
    # left by another chunking, and an allocation size kept from a larger plan, change nothing)
    shape = "576x1984"
    rows, _, max_batch, _ = NAM_SHAPES[shape]
    seed = _one_context_seed(rows, False)  # (test_nam_short_last_chunk's inputs and oracle result)
    nr, pr, ts = _nam_inputs(shape, rows, False, seed)
    dead = np.arange(0, rows, 7)
    o = _nam_oracle(oracle, "every 7th dead", nr, pr, ts, seed, (1, 1), dead, literal=True)
    n1 = 700  # one chunk: the library plans it for 700 pods, with a layout of its own
    o1 = {k: o[k][:n1] for k in ("node", "code", "score", "mask")}  # (no pod's outcome depends on another's)
    with nam._engine(nr, ts, seed, dead=dead, max_batch=max_batch) as e:
        _same(_device_cycle(e, pr[:n1]), o1, "one chunk, first")
        _same(_device_cycle(e, pr), o, "two chunks")
        _same(_device_cycle(e, pr[:n1]), o1, "one chunk, again")
        _same(_device_cycle(e, pr), o, "two chunks, again")


# ---- TaintToleration --------------------------------------------------------------------
TT_NODES, TT_PODS, TT_CUTS = 2100, 700, (0, 37, 38, 900, 2100)  # two row segments; chunks 256/256/188, 7 x 100
TT_CASES = [(kind, mb) for kind in ("sparse", "dense") for mb in (256, 100)]


def _tt_case(oracle, kind):
    def make():
        seed = 33 if kind == "sparse" else 34
        if kind == "sparse":
            nr, pr, dead = tt._cluster(TT_NODES, TT_PODS, seed, dead_every=11)
        else:
            nr, pr = tt._dense_cluster(TT_NODES, TT_PODS, seed)
            dead = np.arange(0, TT_NODES, 9)
        o = _by_pod_slices(lambda p: tt._oracle(oracle, nr, p, seed, dead, literal=True), pr)
        assert (o["code"] == 0).sum() > 0.5 * TT_PODS
        return seed, nr, pr, dead, o
    return _once(("tt", kind), make)


@pytest.mark.parametrize("kind,max_batch", TT_CASES)
def test_tt_chunks_select_device(oracle, kind, max_batch):
    seed, nr, pr, dead, o = _tt_case(oracle, kind)
    with tt._engine(nr, seed, dead=dead, max_batch=max_batch) as e:
        _same(tt._device_cycle(e, pr), o, f"device, max_batch {max_batch}")


@pytest.mark.parametrize("kind,max_batch", TT_CASES)
def test_tt_chunks_host_modes_and_binds(oracle, kind, max_batch):
    seed, nr, pr, dead, o = _tt_case(oracle, kind)
    placed = np.bincount(o["node"][o["code"] == 0], minlength=TT_NODES)
    with tt._engine(nr, seed, dead=dead, max_batch=max_batch) as e:
        _same(e.schedule(pr, _lib.MODE_BATCHED), o, f"host batched, max_batch {max_batch}")
        assert np.array_equal(e.read(0, TT_NODES)["pod_count"], placed)
        _same(e.schedule(pr, _lib.MODE_SEQUENTIAL), o, f"host sequential, max_batch {max_batch}")
        assert np.array_equal(e.read(0, TT_NODES)["pod_count"], 2 * placed)


def _tt_shard_engines(nr, seed, dead, max_batch):
    return [tt._engine(nr, seed, lo, hi, dead, max_batch=max_batch) for lo, hi in zip(TT_CUTS[:-1], TT_CUTS[1:])]


@pytest.mark.parametrize("kind,max_batch", TT_CASES)
def test_tt_chunks_summary_shards(oracle, kind, max_batch):
    # ms_tt_summaries_device per shard (a one-node shard among them), ms_tt_decode_device on each
    import torch

    seed, nr, pr, dead, o = _tt_case(oracle, kind)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    G, P, SB = len(TT_CUTS) - 1, len(pr), _lib.TT_SUMMARY_BYTES
    summ = torch.zeros(G * P * SB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (the fills ran on torch's stream, not s)
    engines = _tt_shard_engines(nr, seed, dead, max_batch)
    try:
        for g, e in enumerate(engines):
            e.tt_summaries_device(P, pods.data_ptr(), summ.data_ptr() + g * P * SB, s.cuda_stream)
        for g, e in enumerate(engines):
            out = torch.full((P * 24,), 0xCD, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            e.tt_decode_device(P, pods.data_ptr(), G, summ.data_ptr(), out.data_ptr(), s.cuda_stream)
            s.synchronize()
            _same(out.cpu().numpy().view(_lib.RESULT), o, f"summaries, max_batch {max_batch}, decoded on {g}")
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("kind,max_batch", TT_CASES)
def test_tt_chunks_two_pass_shards(oracle, kind, max_batch):
    # ms_tt_census_device -> ms_tt_pick_device -> uint64 MAX -> ms_tt_final_device on each shard
    import torch

    seed, nr, pr, dead, o = _tt_case(oracle, kind)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    G, P, CB = len(TT_CUTS) - 1, len(pr), _lib.TT_CENSUS_BYTES
    census = torch.zeros(G * P * CB, dtype=torch.uint8, device=dev)
    keys = torch.zeros((G, P), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # (the fills ran on torch's stream, not s)
    engines = _tt_shard_engines(nr, seed, dead, max_batch)
    try:
        for g, e in enumerate(engines):
            e.tt_census_device(P, pods.data_ptr(), census.data_ptr() + g * P * CB, s.cuda_stream)
        for g, e in enumerate(engines):
            e.tt_pick_device(P, pods.data_ptr(), G, g, census.data_ptr(), keys[g].data_ptr(), s.cuda_stream)
        s.synchronize()
        best = keys.max(dim=0).values.contiguous()  # keys < 2^63: the signed max is the unsigned one
        torch.cuda.synchronize()
        for g, e in enumerate(engines):
            out = torch.full((P * 24,), 0xCD, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            e.tt_final_device(P, pods.data_ptr(), G, census.data_ptr(), best.data_ptr(), out.data_ptr(), s.cuda_stream)
            s.synchronize()
            _same(out.cpu().numpy().view(_lib.RESULT), o, f"two-pass, max_batch {max_batch}, decoded on {g}")
    finally:
        for e in engines:
            e.close()


# ---- NU + NN + NodeAffinity (one term) --------------------------------------------------
@pytest.mark.parametrize("n_nodes", [300, 5000])
def test_na_chunks_device_and_host(oracle, n_nodes):
    # 900 pods at max_batch 256 (chunks 256/256/256/132), weights (3, 2): the chunked sweep +
    # decode of ms_select_batch_device, and ms_schedule_batch with its binds
    seed, n_pods, weights = 40 + n_nodes % 11, 900, (3, 2)
    nr = synth.nodes(n_nodes, seed=seed, zones=True)
    pr = synth.pods(n_pods, seed=seed, zones=True)
    pr["tolerates_unschedulable"][::6] = 1
    pr["name_digit"][::17] = -1
    nr["name_digit"][::9] = 0xFF
    dead = np.arange(3, n_nodes, 10)
    x = nr.copy()
    x["allowed_pods"][dead] = -1
    o = oracle.schedule_na(x, pr, weights=weights, literal=n_nodes <= 300, seed=seed)
    placed = np.bincount(o["node"][o["code"] == 0], minlength=n_nodes)
    with _lib.Engine(max_nodes=n_nodes, plugin_set=_lib.PLUGINS_NU_NN_NA, seed=seed, score_weights=weights,
                     max_batch=256) as e:
        e.upsert(np.arange(n_nodes), nr)
        e.delete(dead.astype(np.uint32))
        e.flush()
        _same(_device_cycle(e, pr), o, "device")
        assert not e.read(0, n_nodes)["pod_count"].any()  # (the device entry point commits no bind)
        _same(e.schedule(pr, _lib.MODE_BATCHED), o, "host batched")
        assert np.array_equal(e.read(0, n_nodes)["pod_count"], placed)
        _same(e.schedule(pr, _lib.MODE_SEQUENTIAL), o, "host sequential")
        assert np.array_equal(e.read(0, n_nodes)["pod_count"], 2 * placed)
    assert (o["code"] == 0).sum() > 0.8 * n_pods


# ---- NU + NN above the fused-launch row limit -------------------------------------------
PP_NODES, PP_PODS = 123_000, 700  # (ms_sweep_pp.hip kPpMaxFusedRows = 122,880)


def _pp_case(oracle):
    def make():
        seed = 47
        nr = synth.nodes(PP_NODES, seed=seed)
        pr = synth.pods(PP_PODS, seed=seed)
        pr["tolerates_unschedulable"][::4] = 1
        pr["name_digit"][::13] = -1
        dead = np.arange(5, PP_NODES, 17)
        x = nr.copy()
        x["allowed_pods"][dead] = -1
        o = oracle.schedule_nunn_omp(x, pr, seed=seed, threads=cpu_threads())
        # winners all over the table, so the combine of a pod's row chunks is in play
        won = o["node"][o["code"] == 0]
        assert len(won) > 0.9 * PP_PODS and all(((won >= a) & (won < a + 41_000)).any() for a in (0, 41_000, 82_000))
        return seed, nr, pr, dead, o
    return _once("pp", make)


@pytest.mark.parametrize("max_batch", [256, 1 << 16])
def test_nunn_chunks_above_fused_limit(oracle, max_batch):
    # chunks 256/256/188 (and one chunk at the default): per chunk several workgroups per pod
    # combine into the key scratch, then a decode
    seed, nr, pr, dead, o = _pp_case(oracle)
    with _lib.Engine(max_nodes=PP_NODES, seed=seed, max_batch=max_batch) as e:
        e.upsert(np.arange(PP_NODES), nr)
        e.delete(dead.astype(np.uint32))
        e.flush()
        _same(_device_cycle(e, pr), o, f"123k rows, max_batch {max_batch}")
