"""MS_PLUGINS_NU_NN_NAM on the GPU: NodeAffinity with
several preferred terms, raw scores up to 400, normalised by RunScorePlugins'
in-loop DefaultNormalizeScore(reverse=false) hook exactly as written, against
the oracle's LITERAL O(F^2) loop: on one context (device and host entry
points, row segments of one context composing their rescale tables) and over
node shards (ms_nam_segment_device -> gather -> ms_nam_keys_device -> uint64
MAX -> ms_decode_device). Reference: /root/reference/minisched/minisched.go:
115-151 (filter), :164-185 (the in-loop hook), :304-325 (selectHost).
"""
import numpy as np
import pytest

from minisched_amd import _lib, synth

pytestmark = pytest.mark.gpu

NAM = _lib.PLUGINS_NU_NN_NAM


def _same(res, o, tag):
    for k_res, k_or in (("node", "node"), ("code", "code"), ("score", "score"), ("plugin_mask", "mask")):
        got, want = np.asarray(res[k_res]).astype(np.int64), np.asarray(o[k_or]).astype(np.int64)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0][:8]
            raise AssertionError(f"{tag} {k_res} differs at {bad.tolist()}: gpu {got[bad].tolist()} "
                                 f"oracle {want[bad].tolist()}")


def _cluster(n_nodes, n_pods, n_sets, seed):
    nr = synth.nodes(n_nodes, seed=seed, labels=True)
    pr = synth.pods(n_pods, seed=seed, term_sets=n_sets)
    pr["name_digit"][::23] = -1
    pr["tolerates_unschedulable"][::9] = 1
    return nr, pr, synth.nam_term_sets(n_sets, seed=seed)


def _ext(ts):
    return np.asarray(ts).ndim == 2 and np.asarray(ts).shape[1] == _lib.NAM_SET_EXT_BYTES


def _oracle(oracle, nr, pr, ts, seed, weights=(1, 1), dead=()):
    # the literal loop is O(F^2) per pod: up to 3,000 nodes; above, its closed form
    # (checked against the loop in tests/test_oracle_nam.py and here on the small ones)
    nr = nr.copy()
    if len(dead):
        nr["allowed_pods"][np.asarray(dead)] = -1
    run = oracle.schedule_nam_ext if _ext(ts) else oracle.schedule_nam
    return run(nr, pr, ts, weights=weights, literal=len(nr) <= 3000, seed=seed)


def _engine(nr, ts, seed, lo=0, hi=None, dead=(), weights=(0, 0), max_batch=1 << 16):
    hi = len(nr) if hi is None else hi
    e = _lib.Engine(max_nodes=max(1, hi - lo), plugin_set=NAM, node_base=lo, seed=seed, score_weights=weights,
                    max_batch=max_batch)
    if _ext(ts):
        e.nam_term_sets_ext(ts)
    else:
        e.nam_term_sets(ts)
    e.upsert(np.arange(lo, hi), nr[lo:hi])
    gone = np.asarray([d for d in dead if lo <= d < hi], dtype=np.uint32)
    if len(gone):
        e.delete(gone)
    e.flush()
    return e


def _device_cycle(e, pr):
    import torch

    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    out = torch.full((len(pr) * 24,), 0xCD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (the fill ran on torch's stream, not s)
    e.select_batch_device(len(pr), pods.data_ptr(), out.data_ptr(), s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy().view(_lib.RESULT)


@pytest.mark.parametrize("n_nodes,n_pods,n_sets,seed", [(1, 40, 3, 1), (7, 200, 5, 2), (300, 500, 24, 3),
                                                        (2100, 300, 40, 4), (9000, 400, 64, 5)])
def test_nam_against_literal_loop(oracle, n_nodes, n_pods, n_sets, seed):
    # one context; 9000 rows = 5 row segments whose rescale tables compose
    nr, pr, ts = _cluster(n_nodes, n_pods, n_sets, seed)
    o = _oracle(oracle, nr, pr, ts, seed)
    with _engine(nr, ts, seed) as e:
        _same(_device_cycle(e, pr), o, f"{n_nodes}x{n_pods}")


@pytest.mark.parametrize("weights", [(2, 1), (1, 3), (7, 5)])
def test_nam_weights_and_tombstones(oracle, weights):
    seed = 20 + weights[0]
    nr, pr, ts = _cluster(5000, 600, 32, seed)
    dead = np.arange(0, 5000, 7)
    o = _oracle(oracle, nr, pr, ts, seed, weights, dead)
    with _engine(nr, ts, seed, dead=dead, weights=weights) as e:
        _same(_device_cycle(e, pr), o, f"weights {weights}")


def test_nam_host_api_chunks_and_binds(oracle):
    # ms_schedule_batch on host arrays in chunks of max_batch pods, binds committed
    seed = 31
    nr, pr, ts = _cluster(3000, 2500, 16, seed)
    o = _oracle(oracle, nr, pr, ts, seed)
    with _engine(nr, ts, seed, max_batch=1000) as e:
        _same(e.schedule(pr, _lib.MODE_BATCHED), o, "host api")
        tab = e.read(0, 3000)
        cnt = np.bincount(o["node"][o["code"] == 0], minlength=3000)
        assert np.array_equal(tab["pod_count"], cnt)


def test_nam_term_sets_can_be_replaced(oracle):
    seed = 41
    nr, pr, ts = _cluster(800, 300, 10, seed)
    ts2 = synth.nam_term_sets(10, seed=seed + 1)
    with _engine(nr, ts, seed) as e:
        _same(_device_cycle(e, pr), _oracle(oracle, nr, pr, ts, seed), "sets 1")
        e.nam_term_sets(ts2)
        _same(_device_cycle(e, pr), _oracle(oracle, nr, pr, ts2, seed), "sets 2")
        with pytest.raises(_lib.MSError):
            e.nam_term_sets(np.full((1, 16), 200, dtype=np.uint8))  # key 200: rejected


@pytest.mark.parametrize("cuts", [(0, 4500, 9000), (0, 37, 38, 4000, 9000), (0, 3, 6000)])
def test_nam_node_shards(oracle, cuts):
    # node shards: per-shard rescale records, gathered shard-major; each shard's keys
    # under the later shards' rescales and the cluster's anchor; uint64 MAX; decode.
    # Includes a one-node shard, a shard with every node deleted, tiny shards
    import torch

    seed = 50 + len(cuts)
    n = cuts[-1]
    nr, pr, ts = _cluster(n, 1500, 48, seed)
    dead = np.arange(cuts[1], cuts[2]) if len(cuts) > 3 else np.arange(0, n, 13)
    o = _oracle(oracle, nr, pr, ts, seed, dead=dead)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    G, P, SB = len(cuts) - 1, len(pr), _lib.NAM_SEG_BYTES
    segs = torch.zeros(G * P * SB, dtype=torch.uint8, device=dev)
    keys = torch.zeros((G, P), dtype=torch.int64, device=dev)
    out = torch.zeros(P * 24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (the fills ran on torch's stream, not s)
    engines = [_engine(nr, ts, seed, lo, hi, dead) for lo, hi in zip(cuts[:-1], cuts[1:])]
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
        _same(out.cpu().numpy().view(_lib.RESULT), o, f"shards {cuts}")
        with pytest.raises(_lib.MSError):  # keys alone do not combine for this set
            kb = torch.zeros(P, dtype=torch.int64, device=dev)
            engines[0].sweep_device(P, pods.data_ptr(), kb.data_ptr(), 0, s.cuda_stream)
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("key", [0, 1])
def test_nam_label_id_255_matches_exists(oracle, key):
    # a node label id of 255 is a labelled node, so an Exists term (value 0xFF)
    # must match it as the oracle's nam_raw does; In terms name ids 1..254 (0xFF is Exists)
    nr, pr, _ = _cluster(600, 300, 4, 7)
    field = "zone" if key == 0 else "label2"
    nr[field][::3] = 255
    nr[field][1::7] = 254
    nr[field][2::11] = 0  # unlabelled: never matches
    ts = _lib.nam_term_sets_array([[(key, 0xFF, 40)], [(key, 254, 90), (key, 0xFF, 15)],
                                   [(1 - key, 0xFF, 60), (key, 0xFF, 70), (key, 1, 5)], [(key, 254, 100)]])
    o = _oracle(oracle, nr, pr, ts, 7)
    with _engine(nr, ts, 7) as e:
        _same(_device_cycle(e, pr), o, f"label id 255 on key {key}")



# ---- general terms (ABI 7): In / NotIn / Exists / DoesNotExist / Gt / Lt as value-id sets ----
def _ext_cluster(n_nodes, n_pods, n_sets, seed):
    nr, pr, _ = _cluster(n_nodes, n_pods, n_sets, seed)
    nr["zone"][::17] = 255  # (id 255: a labelled node)
    nr["label2"][5::23] = 255
    return nr, pr, synth.nam_term_sets_ext(n_sets, seed=seed)


@pytest.mark.parametrize("n_nodes,n_pods,n_sets,seed", [(1, 60, 5, 61), (40, 300, 12, 62), (700, 900, 40, 63),
                                                        (2900, 400, 64, 64), (12000, 700, 64, 65)])
def test_nam_ext_against_literal_loop(oracle, n_nodes, n_pods, n_sets, seed):
    nr, pr, ts = _ext_cluster(n_nodes, n_pods, n_sets, seed)
    o = _oracle(oracle, nr, pr, ts, seed)
    with _engine(nr, ts, seed) as e:
        _same(_device_cycle(e, pr), o, f"ext {n_nodes}x{n_pods}")


def test_nam_ext_many_classes_and_unknown_sets(oracle):
    # many sorted classes (at most 2 x 1,201 x 11 digits = 26,422 buckets, within the class
    # sort's 65,536), term set ids past the registered ones (no terms), a chunked host call
    seed = 66
    nr, pr, ts = _ext_cluster(1500, 5000, 1200, seed)
    sid = (np.arange(len(pr)) * 7919) % 1400  # ids 1201..1399: not registered
    pr["pref_zone"], pr["pref_weight"] = sid & 0xFF, sid >> 8
    o = _oracle(oracle, nr, pr, ts, seed)
    with _engine(nr, ts, seed) as e:
        _same(_device_cycle(e, pr), o, "many classes")
    with _engine(nr, ts, seed, max_batch=1700) as e:
        _same(e.schedule(pr, _lib.MODE_BATCHED), o, "many classes, host chunks")


def test_nam_ext_more_classes_than_the_class_sort_holds(oracle):
    # 3,200 sets: all 6,400 (set, toleration) classes in ONE chunk, 6,402 x 11 = 70,422 buckets
    # past the class sort's 65,536, so the pods keep batch order (ctl[1] == 0, rep[c] by
    # atomicMin, perm[i] = i); 1,600 more pods repeat 40 classes at distant batch positions
    seed = 71
    nr, pr, ts = _ext_cluster(300, 8000, 3200, seed)
    rng = np.random.default_rng(seed)
    cls = np.concatenate([rng.permutation(6400), np.tile(rng.choice(6400, 40, replace=False), 40)])
    cls[6400:] = rng.permutation(cls[6400:])
    cls[[0, 7999]] = cls[[7999, 0]]  # (a repeated class first in the batch, a single one last)
    sid = 1 + cls // 2
    pr["pref_zone"], pr["pref_weight"], pr["tolerates_unschedulable"] = sid & 0xFF, sid >> 8, cls & 1
    assert len(set(cls.tolist())) == 6400 and 6402 * 11 > 65536
    o = _oracle(oracle, nr, pr, ts, seed)
    with _engine(nr, ts, seed) as e:
        _same(_device_cycle(e, pr), o, "unsorted classes, device")
        _same(e.schedule(pr, _lib.MODE_BATCHED), o, "unsorted classes, host")


@pytest.mark.parametrize("weights", [(1, 1), (3, 2)])
def test_nam_ext_node_shards(oracle, weights):
    import torch

    seed = 67 + weights[0]
    cuts = (0, 1, 2200, 2201, 5000)
    n = cuts[-1]
    nr, pr, ts = _ext_cluster(n, 900, 48, seed)
    dead = np.arange(0, n, 11)
    o = _oracle(oracle, nr, pr, ts, seed, weights=weights, dead=dead)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    G, P, SB = len(cuts) - 1, len(pr), _lib.NAM_SEG_BYTES
    segs = torch.zeros(G * P * SB, dtype=torch.uint8, device=dev)
    keys = torch.zeros((G, P), dtype=torch.int64, device=dev)
    out = torch.zeros(P * 24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engines = [_engine(nr, ts, seed, lo, hi, dead, weights=weights) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        for g, e in enumerate(engines):
            e.nam_segment_device(P, pods.data_ptr(), segs.data_ptr() + g * P * SB, s.cuda_stream)
        for g, e in enumerate(engines):
            e.nam_keys_device(P, pods.data_ptr(), G, g, segs.data_ptr(), keys[g].data_ptr(), s.cuda_stream)
        s.synchronize()
        best = keys.max(dim=0).values.contiguous()
        present = sum(int(e.info().present_nodes) for e in engines)
        torch.cuda.synchronize()
        engines[0].decode_device(P, pods.data_ptr(), best.data_ptr(), 0, present, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        _same(out.cpu().numpy().view(_lib.RESULT), o, f"ext shards {weights}")
    finally:
        for e in engines:
            e.close()


def test_nam_ext_rejects_weights_above_100():
    ts = synth.nam_term_sets_ext(2, seed=3)
    ts[1, 64] = 101
    with _lib.Engine(max_nodes=10, plugin_set=NAM, seed=1) as e:
        with pytest.raises(_lib.MSError):
            e.nam_term_sets_ext(ts)
