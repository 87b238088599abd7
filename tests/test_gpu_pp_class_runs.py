"""K1 pp's class-sorted pod runs (ms_sweep_pp.hip: the prologue's counting sort by
(fixed slot, tolerates) and the run form of sweep_range) against the CPU oracle.

The run form needs a workgroup chunk of at least 80 pods (kPpSortMin) holding 8 or
more pods of one class, so every case forces large chunks. From sweep_pp_impl:
with MINISCHED_PP_WAVES=W a workgroup has W waves, and while the chunk stays
<= 1024 pods one round of 16 / W workgroups per CU is resident, so
chunk = roundup8(ceil(n_pods / (CUs * 16 / W))) (grid.y == 1 for every table
here). W = 16 and n_pods = 100 * CUs give chunks of 104 pods; W = 4 takes the
balanced split (chunks of 96 and 104 pods at 400 * CUs - 1 pods on a 256-CU part).
Every case compares node, code, score and plugin mask of every pod.
"""
import numpy as np
import pytest

from minisched_amd import _lib, synth
from minisched_amd._lib import MODE_BATCHED
from test_gpu_parity import assert_same, engine_with, need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _n_pods(waves=16, per_chunk=100):
    # chunks of at least per_chunk pods (module docstring); one host chunk per
    # call (ms_hostarray.cpp splits calls of 100,000 pods and more)
    slots = _cus() * (16 // waves)
    n = min(per_chunk * slots, 99_999)
    assert n // slots // 8 * 8 >= 80, "chunks too small for the class sort"
    return n


def _pods(n, seed):
    pr = synth.pods(n, seed=seed)
    pr["tolerates_unschedulable"] = 0
    pr["tolerates_unschedulable"][::5] = 1
    pr["name_digit"][::13] = -1
    return pr


@pytest.mark.parametrize("node_base", [0, 7, 999_990])
def test_class_runs_base(oracle, monkeypatch, node_base):
    # every digit class of a chunk forms runs; the fixed slot moves with node_base % 10
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    nr = synth.nodes(3000, seed=51, start=node_base)
    pr = _pods(_n_pods(), 51)
    o = oracle.schedule(nr, pr, seed=51, node_base=node_base)
    with engine_with(nr, seed=51, node_base=node_base) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)
    assert (o["score"] == 10).sum() > len(pr) // 2


def test_class_runs_lengths(oracle, monkeypatch):
    # chunk 0: classes of exactly 7, 8, 9, 16 and 17 pods (no run, one whole block,
    # a block and a rest of 1, two blocks, two and a rest) and 47 of a sixth;
    # chunk 1: one single class; the others cycle
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    cus = _cus()
    chunk = 104
    pr = synth.pods(chunk * cus, seed=52)
    pr["tolerates_unschedulable"] = 0
    pr["tolerates_unschedulable"][2 * chunk::5] = 1
    pr["name_digit"][:chunk] = np.repeat(np.arange(6), [7, 8, 9, 16, 17, 47])
    rng = np.random.default_rng(52)
    pr["name_digit"][:chunk] = rng.permutation(pr["name_digit"][:chunk])
    pr["name_digit"][chunk:2 * chunk] = 6
    nr = synth.nodes(3000, seed=52)
    o = oracle.schedule(nr, pr, seed=52)
    with engine_with(nr, seed=52) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)


def test_class_runs_wave_without_candidate(oracle, monkeypatch):
    # no schedulable row of digit 3: its non-tolerating pods find no score-10 row in
    # any wave (no run form, level 1 through pod_slow), tolerating ones do; then a
    # table with every row unschedulable
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    nr = synth.nodes(3000, seed=53)
    nr["unschedulable"][nr["name_digit"] == 3] = 1
    pr = synth.pods(_n_pods(), seed=53)
    pr["tolerates_unschedulable"] = 0
    pr["tolerates_unschedulable"][::7] = 1
    o = oracle.schedule(nr, pr, seed=53)
    with engine_with(nr, seed=53) as e:
        res = e.schedule(pr, MODE_BATCHED)
    assert_same(res, o)
    d3 = pr["name_digit"] == 3
    tol = pr["tolerates_unschedulable"] == 1
    assert np.all(res["score"][d3 & ~tol] == 0) and np.all(res["code"][d3 & ~tol] == 0)
    assert np.all(res["score"][d3 & tol] == 10)
    nr["unschedulable"] = 1
    o = oracle.schedule(nr, pr, seed=53)
    with engine_with(nr, seed=53) as e:
        res = e.schedule(pr, MODE_BATCHED)
    assert_same(res, o)
    assert np.all(res["code"][~tol] == 2) and np.all(res["score"][tol] == 10)


def test_class_runs_lanes_without_candidate(oracle, monkeypatch):
    # 90 % tombstones (test_fixed_slot_form's sparse layout): most lanes hold no row
    # of a class and borrow another lane's candidate base
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    n = 40_000
    nr = synth.nodes(n, seed=54)
    rng = np.random.default_rng(54)
    nr["allowed_pods"][rng.random(n) < 0.9] = -1
    pr = _pods(_n_pods(), 54)
    o = oracle.schedule(nr, pr, seed=54)
    with engine_with(nr, seed=54) as e:
        e.delete(np.flatnonzero(nr["allowed_pods"] < 0).astype(np.uint32))
        assert_same(e.schedule(pr, MODE_BATCHED), o)
    assert (o["code"] == 0).sum() > 0


def test_class_runs_mixed_workgroup(oracle, monkeypatch):
    # 6,000 rows are 200 groups, 64 to a wave: group 166 (row 5,000, wave 2) is
    # misaligned, so that wave takes the slot search and waves 0 and 3 the fixed
    # slots, all three in the run form; group 100 (wave 1) is over-full: the
    # bit-scan loop, no run form
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    nr = synth.nodes(6000, seed=55)
    nr["name_digit"][5000] = (nr["name_digit"][5000] + 1) % 10
    nr["name_digit"][3000:3030] = 4
    pr = _pods(_n_pods(), 55)
    o = oracle.schedule(nr, pr, seed=55)
    with engine_with(nr, seed=55) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)


@pytest.mark.parametrize("rows", [2100, 9630])
def test_class_runs_packed_last_word(oracle, monkeypatch, rows):
    # 4-wave workgroups pack a last word of <= 8 groups (tail_pods): 2,100 rows are
    # 70 groups, one full word and a 6-group tail, 9,630 rows 321, five words and
    # one group; the packed word is evaluated per pod beside the run form, and the
    # balanced split gives chunks of two sizes
    monkeypatch.setenv("MINISCHED_PP_WAVES", "4")
    nr = synth.nodes(rows, seed=56)
    pr = _pods(_n_pods(waves=4), 56)
    o = oracle.schedule(nr, pr, seed=56)
    with engine_with(nr, seed=56) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)


def test_class_runs_output_forms(oracle, monkeypatch):
    # the epilogue writes by the entry's original index: the decoded results with
    # the bind commit, the compact records, and the packed keys
    import torch

    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    n, seed = 6000, 57
    nr = synth.nodes(n, seed=seed)
    pr = _pods(_n_pods(), seed)
    o = oracle.schedule(nr, pr, seed=seed)
    placed = np.bincount(o["node"][o["code"] == 0], minlength=n)
    with engine_with(nr, seed=seed) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)
        assert np.array_equal(e.read(0, n)["pod_count"], placed)
        r = e.schedule_compact(_lib.compact_pods(pr))
        for k_res, k_or in (("node", "node"), ("code", "code"), ("score", "score"), ("plugin_mask", "mask")):
            assert np.array_equal(r[k_res].astype(np.int64), o[k_or].astype(np.int64)), k_res
        assert np.array_equal(e.read(0, n)["pod_count"], 2 * placed)
        dev = torch.device("cuda:0")
        s = torch.cuda.Stream(device=dev)
        pods_d = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
        keys = torch.empty(len(pr), dtype=torch.int64, device=dev)
        res_d = torch.empty(len(pr) * 24, dtype=torch.uint8, device=dev)
        e.sweep_device(len(pr), pods_d.data_ptr(), keys.data_ptr(), 0, s.cuda_stream)
        e.select_batch_device(len(pr), pods_d.data_ptr(), res_d.data_ptr(), s.cuda_stream)
        s.synchronize()
    k = keys.cpu().numpy().view(np.uint64)
    assert np.array_equal(np.where(k <= 1, 0, k), o["key"]) and np.array_equal(k == 1, o["key"] == 0)
    assert_same(res_d.cpu().numpy().view(_lib.RESULT), o)


def test_class_runs_two_workgroups_per_chunk(oracle):
    # more than 122,880 rows: two workgroups (grid.y) sweep each chunk, each sorts it
    # on its own (the order inside a class differs) and both combine by atomicMax on
    # the pod's original index. Half a round of workgroups per chunk row, so
    # chunk = roundup8(n_pods / (CUs / 2)) = 104. (The OpenMP oracle: 1.6e9 pairs.)
    nr = synth.nodes(123_000, seed=58)
    pr = _pods(50 * _cus(), 58)
    o = oracle.schedule_nunn_omp(nr, pr, seed=58)
    with engine_with(nr, seed=58) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)


def _zero_hash_pods(seed, n_nodes, want=4):
    # (pod ordinal j, node ordinal r < n_nodes) with tie-break hash exactly 0, distinct
    # digits r % 10: mix32 is a bijection fixing 0, so r = -A * kG24^-1 mod 2^32
    # (test_gpu_parity._pods_with_zero_hash, searching on past its first 2^20 pods)
    import _pyref

    M = np.uint64(0xFFFFFFFF)

    def fmix32(h):
        h = h ^ (h >> np.uint64(16))
        h = (h * np.uint64(0x85EBCA6B)) & M
        h = h ^ (h >> np.uint64(13))
        h = (h * np.uint64(0xC2B2AE35)) & M
        return h ^ (h >> np.uint64(16))

    out, digits = [], set()
    with np.errstate(over="ignore"):
        for j0 in range(0, 1 << 26, 1 << 20):
            js = np.arange(j0, j0 + (1 << 20), dtype=np.uint64)
            a = fmix32(js ^ np.uint64(_pyref.seed32(seed)))
            r = (((M + np.uint64(1) - a) & M) * np.uint64(0xF2B382C9)) & M
            for x in np.nonzero(r < np.uint64(n_nodes))[0]:
                rr = int(r[x])
                if rr % 10 not in digits and len(out) < want:
                    assert _pyref.h32(seed, int(js[x]), rr) == 0
                    digits.add(rr % 10)
                    out.append((int(js[x]), rr))
            if len(out) == want:
                return out
    raise AssertionError("no zero-hash pods found")


def test_class_runs_zero_hash_winner(oracle, monkeypatch):
    # test_pp_zero_hash_winner at a run-forming shape: chunk 0 holds 8 pods of each
    # of the 8 (digit, tolerates) classes of the zero-hash pods (whole blocks, so
    # each is swept in the run form wherever the sort puts it) and 40 of another
    # digit. Alone, the zero-hash row fills every slot, the maximum is 0 and the pod
    # is redone exactly; beside other score-10 rows the 0 loses. (8,192 rows, five
    # waves with rows, where that test has 32,768: the oracle's time)
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    seed, n = 4, 1 << 13
    cases = _zero_hash_pods(seed, n)
    nr = synth.nodes(n, seed=seed)
    nr["unschedulable"] = 0
    pr = synth.pods(_n_pods(), seed=seed, start=1 << 27)
    pr["tolerates_unschedulable"] = 0
    pr["tolerates_unschedulable"][104::5] = 1
    spare = min(set(range(10)) - {r % 10 for _, r in cases})
    pr["name_digit"][64:104] = spare
    for k, (j, r) in enumerate(cases):
        for t in (0, 1):
            blk = slice(16 * k + 8 * t, 16 * k + 8 * t + 8)
            pr["name_digit"][blk] = r % 10
            pr["tolerates_unschedulable"][blk] = t
            pr["ordinal"][16 * k + 8 * t + 3] = j
    lone = nr.copy()
    for j, r in cases:  # every other node of that digit unschedulable
        same = (np.arange(n) % 10 == r % 10) & (np.arange(n) != r)
        lone["unschedulable"][same] = 1
    for table, tag in ((lone, "lone"), (nr, "crowded")):
        o = oracle.schedule(table, pr, seed=seed)
        with engine_with(table, seed=seed) as e:
            res = e.schedule(pr, MODE_BATCHED)
        assert_same(res, o)
        if tag == "lone":
            for k, (j, r) in enumerate(cases):
                assert res["node"][16 * k + 3] == r and res["score"][16 * k + 3] == 10, (j, r)
