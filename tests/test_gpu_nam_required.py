"""NodeAffinity as a filter (nodeSelector and required terms,
ms_nam_required_sets) in MS_PLUGINS_NU_NN_NAM on the GPU: node, code, score and
FitError mask element for element against the tombstone reference of
tests/_nam_required_ref.py (the C oracle on a table whose rows failing the
requirement are dead, the mask recomputed), which tests/test_nam_required.py
checks against the literal Python restatement on these same inputs. One
context (device and host entry points), table handling, and node shards
(ms_nam_segment_device -> gather -> ms_nam_keys_device -> uint64 MAX,
ms_nam_flags_device -> ms_decode_device with flags).
"""
import numpy as np
import pytest

import _nam_required_cases as cases
import _nam_required_ref as ref
from minisched_amd import _lib, synth

pytestmark = pytest.mark.gpu

NAM = _lib.PLUGINS_NU_NN_NAM
NO_REQ = _lib.nam_required_sets_array([])


def _engine(nr, ts, rq, seed, lo=0, hi=None, dead=(), weights=(0, 0), max_batch=1 << 16):
    hi = len(nr) if hi is None else hi
    e = _lib.Engine(max_nodes=max(1, hi - lo), plugin_set=NAM, node_base=lo, seed=seed, score_weights=weights,
                    max_batch=max_batch)
    e.nam_term_sets_ext(ts)
    e.nam_required_sets(rq)
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


def _want(oracle, nr, pr, ts, rq, seed, weights=(1, 1), dead=()):
    return ref.schedule_tombstone(oracle, nr, pr, ts, rq, weights=weights, seed=seed, dead=dead)


def test_inputs_cover_every_mask_and_a_moved_winner(oracle):
    # the reference itself must yield every FitError mask (1, 8, 9) and a SUCCESS whose
    # winner the filter moved, or the comparisons below would not show them
    total, moved = {1: 0, 8: 0, 9: 0}, 0
    runs = [cases.cluster(*s) + (s[3],) for s in cases.SHAPES] + [cases.all_unschedulable_case()]
    for nr, pr, ts, rq, seed in runs:
        m, mv = cases.coverage(_want(oracle, nr, pr, ts, rq, seed), _want(oracle, nr, pr, ts, NO_REQ, seed))
        total = {k: total[k] + m[k] for k in total}
        moved += mv
    assert min(total.values()) >= 1 and moved >= 1, (total, moved)


@pytest.mark.parametrize("n_nodes,n_pods,n_sets,seed", cases.SHAPES)
def test_one_context_against_reference(oracle, n_nodes, n_pods, n_sets, seed):
    nr, pr, ts, rq = cases.cluster(n_nodes, n_pods, n_sets, seed)
    with _engine(nr, ts, rq, seed) as e:
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts, rq, seed), f"{n_nodes}x{n_pods}")


def test_hand_cases(oracle):
    # the anchor moves and a rescale disappears: 70 + 33 unfiltered, 70 + 40 filtered
    nr, pr, ts, rq = cases.inloop_cluster()
    with _engine(nr, ts, NO_REQ, 1, weights=(7, 1)) as e:
        res = _device_cycle(e, pr)
        assert res["node"].tolist() == [0] * 4 and res["score"].tolist() == [103] * 4
        e.nam_required_sets(rq)
        res = _device_cycle(e, pr)
        assert res["node"].tolist() == [0] * 4 and res["score"].tolist() == [110] * 4
    # every node unschedulable: mask 1 alone for the pods that do not tolerate it
    nr, pr, ts, rq, seed = cases.all_unschedulable_case()
    want = _want(oracle, nr, pr, ts, rq, seed)
    assert cases.coverage(want, want)[0][1] >= 1
    with _engine(nr, ts, rq, seed) as e:
        ref.same(_device_cycle(e, pr), want, "all unschedulable")
    # no node listed: an empty mask
    with _lib.Engine(max_nodes=8, plugin_set=NAM, seed=1) as e:
        e.nam_required_sets(rq)
        res = _device_cycle(e, pr)
        assert set(res["code"].tolist()) == {2} and set(res["plugin_mask"].tolist()) == {0}


@pytest.mark.parametrize("weights", cases.WEIGHTS)
def test_weights_and_tombstones(oracle, weights):
    nr, pr, ts, rq, dead, seed = cases.weights_case(weights)
    with _engine(nr, ts, rq, seed, dead=dead, weights=weights) as e:
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts, rq, seed, weights, dead), f"weights {weights}")


def test_host_api_chunks_and_binds(oracle):
    # ms_schedule_batch in chunks of max_batch pods (a short last chunk), binds committed
    nr, pr, ts, rq, seed = cases.host_case()
    want = _want(oracle, nr, pr, ts, rq, seed)
    with _engine(nr, ts, rq, seed, max_batch=1000) as e:
        ref.same(e.schedule(pr, _lib.MODE_BATCHED), want, "host api")
        cnt = np.bincount(want["node"][want["code"] == 0], minlength=len(nr))
        assert np.array_equal(e.read(0, len(nr))["pod_count"], cnt)


def test_tables_are_installed_independently(oracle):
    seed = 41
    nr, pr, ts, rq = cases.cluster(800, 300, 10, seed)
    ts2, rq2 = synth.nam_term_sets_ext(10, seed=seed + 1), synth.nam_required_sets(10, seed=seed + 1)
    with _engine(nr, ts, rq, seed) as e:
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts, rq, seed), "first tables")
        e.nam_required_sets(rq2)  # replacing the required table keeps the preferred one
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts, rq2, seed), "required replaced")
        e.nam_term_sets_ext(ts2)  # and the reverse
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts2, rq2, seed), "preferred replaced")
        # more required ids than preferred ids, and the reverse: ids past a table have none of its kind
        e.nam_term_sets_ext(ts2[:4])
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts2[:4], rq2, seed), "4 preferred, 10 required")
        e.nam_term_sets_ext(ts2)
        e.nam_required_sets(rq2[:3])
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts2, rq2[:3], seed), "10 preferred, 3 required")
        e.nam_term_sets_ext(ts2[:0])
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts2[:0], rq2[:3], seed), "required only")
        # a set with five terms is refused, and the registered table stays
        bad = rq2.copy()
        bad[1, 256] = 5
        with pytest.raises(_lib.MSError) as err:
            e.nam_required_sets(bad)
        assert err.value.code == _lib.MS_E_INVAL
        ref.same(_device_cycle(e, pr), _want(oracle, nr, pr, ts2[:0], rq2[:3], seed), "after the refusal")
        # clearing restores the results without the feature: the oracle's own, mask included
        e.nam_term_sets_ext(ts)
        e.nam_required_sets(NO_REQ)
        ref.same(_device_cycle(e, pr), oracle.schedule_nam_ext(nr, pr, ts, literal=True, seed=seed), "cleared")


@pytest.mark.parametrize("cuts", cases.SHARD_CUTS)
def test_node_shards(oracle, cuts):
    # per-shard records (now with the shard's filter bits), gathered shard-major; keys under the
    # later shards' rescales; uint64 MAX; the filter bits ORed over the shards; decode with flags.
    # Includes a one-node shard and a shard with every node deleted.
    import torch

    nr, pr, ts, rq, dead, seed = cases.shard_case(cuts)
    want = _want(oracle, nr, pr, ts, rq, seed, dead=dead)
    assert ((want["code"] == 2) & (want["mask"] != 1)).any()  # (a NodeAffinity FitError: the flags matter)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    G, P, SB = len(cuts) - 1, len(pr), _lib.NAM_SEG_BYTES
    segs = torch.zeros(G * P * SB, dtype=torch.uint8, device=dev)
    keys = torch.zeros((G, P), dtype=torch.int64, device=dev)
    flags = torch.full((P,), -1, dtype=torch.int32, device=dev)
    out = torch.zeros(P * 24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (the fills ran on torch's stream, not s)
    engines = [_engine(nr, ts, rq, seed, lo, hi, dead) for lo, hi in zip(cuts[:-1], cuts[1:])]
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
        ref.same(out.cpu().numpy().view(_lib.RESULT), want, f"shards {cuts}")
    finally:
        for e in engines:
            e.close()
