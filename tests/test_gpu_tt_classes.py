"""MS_PLUGINS_NU_TT_NN on the GPU with the biased clusters of tests/_tt_cases.py,
in which every count class 0..8 (with and without a NodeNumber match) and every
explicit entry (feasible ranks 0, 1, 2 and the last row) wins for many pods;
tests/test_tt_cases.py counts them and proves the inputs' model against the C
oracle. The same clusters go through four paths and all four result fields are
compared exactly with the oracle (its literal loop up to 40 rows, its closed
form above): select_batch_device, the host call, the summary path over node
shards (tt_summaries_device / tt_decode_device) and the two-pass path over
shards (tt_census_device / tt_pick_device / max / tt_final_device). The shard
cuts leave a first shard of two or three rows (fewer than four feasible rows)
and a second cut at an odd row, so that the feasible count before a shard is
odd for some pods and even for others.
"""
import numpy as np
import pytest

import _tt_cases as tc
from minisched_amd import _lib

pytestmark = pytest.mark.gpu

TT = _lib.PLUGINS_NU_TT_NN


def _same(res, o, tag):
    for k_res, k_or in (("node", "node"), ("code", "code"), ("score", "score"), ("plugin_mask", "mask")):
        got, want = np.asarray(res[k_res]).astype(np.int64), np.asarray(o[k_or]).astype(np.int64)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0][:8]
            raise AssertionError(f"{tag} {k_res} differs at {bad.tolist()}: gpu {got[bad].tolist()} "
                                 f"oracle {want[bad].tolist()}")


def _engine(nr, lo=0, hi=None):
    hi = len(nr) if hi is None else hi
    e = _lib.Engine(max_nodes=max(1, hi - lo), plugin_set=TT, node_base=lo, seed=tc.SEED)
    e.upsert(np.arange(lo, hi), nr[lo:hi])
    e.flush()
    return e


def _cuts(n):
    return (0, 2, n // 2 + 1, n) if n <= 40 else (0, 3, 1031, n)


def _four_paths(oracle, n, variant):
    import torch

    nr, pr = tc.cluster(n, variant)
    o = oracle.schedule_tt(nr, pr, literal=n <= 40, seed=tc.SEED)
    tag = f"{n} rows, variant {variant}"
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    P = len(pr)

    def fresh():
        out = torch.full((P * 24,), 0xCD, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (the fill ran on torch's stream, not s)
        return out

    def result(out):
        s.synchronize()
        return out.cpu().numpy().view(_lib.RESULT)

    with _engine(nr) as e:
        out = fresh()
        e.select_batch_device(P, pods.data_ptr(), out.data_ptr(), s.cuda_stream)
        _same(result(out), o, tag + ", device")
        _same(e.schedule(pr, _lib.MODE_BATCHED), o, tag + ", host")
    cuts = _cuts(n)
    G, SB, CB = len(cuts) - 1, _lib.TT_SUMMARY_BYTES, _lib.TT_CENSUS_BYTES
    summ = torch.zeros(G * P * SB, dtype=torch.uint8, device=dev)
    census = torch.zeros(G * P * CB, dtype=torch.uint8, device=dev)
    keys = torch.zeros((G, P), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    engines = [_engine(nr, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        for g, e in enumerate(engines):
            e.tt_summaries_device(P, pods.data_ptr(), summ.data_ptr() + g * P * SB, s.cuda_stream)
        out = fresh()
        engines[-1].tt_decode_device(P, pods.data_ptr(), G, summ.data_ptr(), out.data_ptr(), s.cuda_stream)
        _same(result(out), o, tag + f", summaries over shards {cuts}")
        for g, e in enumerate(engines):
            e.tt_census_device(P, pods.data_ptr(), census.data_ptr() + g * P * CB, s.cuda_stream)
        for g, e in enumerate(engines):
            e.tt_pick_device(P, pods.data_ptr(), G, g, census.data_ptr(), keys[g].data_ptr(), s.cuda_stream)
        s.synchronize()
        best = keys.max(dim=0).values.contiguous()  # keys < 2^63: the signed max is the unsigned one
        out = fresh()
        engines[1].tt_final_device(P, pods.data_ptr(), G, census.data_ptr(), best.data_ptr(), out.data_ptr(),
                                   s.cuda_stream)
        _same(result(out), o, tag + f", two passes over shards {cuts}")
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("n", tc.SMALL_SIZES)
def test_small_lists_on_four_paths(oracle, n):
    for _, variant in tc.clusters((n,)):
        _four_paths(oracle, n, variant)


@pytest.mark.parametrize("n", tc.LARGE_SIZES)
def test_large_lists_on_four_paths(oracle, n):
    for _, variant in tc.clusters((n,)):
        _four_paths(oracle, n, variant)
