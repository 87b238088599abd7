"""K1 pp's lane table (ms_sweep_pp.hip: table_put, table_rowmax, lane_table_fits) against
the CPU oracle.

In the list form a wave no longer reduces its lane maxima per 8-pod block: it puts them
into the pod's row of a u32 table in LDS (64 words per pod position, one ds_max_u32 per
pod), and after the sweep the workgroup reduces each row once. A row's maximum is level 11
whatever its value, so which pods take it is decided by class (the digit's lists hold a
tile for the pod's toleration), not by the value; the other pods keep what the planes path
left in their slot. The host takes the table form where the chunk is swept in the list
form and the workgroup's LDS with the table still lets the workgroups the chunk was sized
for stay resident (_table_fits restates lane_table_fits); else the per-wave reduction
runs as before.

The cases force list-form chunks as test_gpu_pp_shared_lists.py does (MINISCHED_PP_WAVES,
about 100 pods per chunk) and compare node, code, score and plugin mask of every pod; each
also asserts from the oracle's own result what it was built to show.
"""
import numpy as np
import pytest

from minisched_amd import _lib, synth
from minisched_amd._lib import MODE_BATCHED
from test_gpu_parity import assert_same, engine_with, need_gpu  # noqa: F401
from test_gpu_pp_class_runs import _cus, _n_pods, _zero_hash_pods
from test_gpu_pp_shared_lists import _assert_cordoned_only_tolerated, _mixed_pods, _run_mixed, _split_table

pytestmark = pytest.mark.gpu

LANE_WORDS = 64  # kPpLaneWords
LDS_PER_CU = 160 * 1024


def _lds_bytes(cap, lane_words):
    # pp_lds_bytes: 8-byte slots and entries, 96 sort words, the table
    return cap * 16 + 96 * 4 + cap * lane_words * 4


def _table_fits(chunk, xtra, waves, per_cu):
    # lane_table_fits: a sorted chunk, and per_cu workgroups of it (2 KiB granules) in a CU
    if chunk < 80 or waves > 16:
        return False
    wg = -(-_lds_bytes(chunk + (8 if xtra else 0), LANE_WORDS) // 2048) * 2048
    return wg * per_cu <= LDS_PER_CU


@pytest.mark.parametrize("waves", [16, 4])
def test_lane_table_both_shapes(oracle, monkeypatch, waves):
    # 16-wave workgroups, one to a CU, and 4-wave ones, four to a CU (the balanced split,
    # chunks of two sizes); pods of both tolerations in every digit, some without a digit
    assert _table_fits(104, 0, 16, 1) and _table_fits(96, 1, 4, 4)
    nr = synth.nodes(3000, seed=81)
    pr, o = _run_mixed(oracle, monkeypatch, nr, waves, 81)
    d, tol = pr["name_digit"], pr["tolerates_unschedulable"] == 1
    for dg in range(10):
        assert ((d == dg) & tol).sum() > 0 and ((d == dg) & ~tol).sum() > 0
    assert (d < 0).sum() > 0 and np.all(o["score"][d >= 0] == 10) and np.all(o["score"][d < 0] == 0)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("waves,rows", [(16, 13_500), (4, 3_600)])
def test_uneven_digits(oracle, monkeypatch, waves, rows):
    # digit 3: S holds 100 rows more than one pass of 4 x waves tiles and U 100 rows, so the
    # second pass holds an S tile (wave 0) and the U tile (wave 1): pods of both kinds are
    # swept in two passes that meet in their rows of the table. (16 waves need 12,388
    # schedulable rows of one digit for that, hence the larger table.) Digit 7: a single
    # row, so its tile is that entry and 191 copies, and 15 of 16 waves write nothing.
    one_pass = 4 * waves * 192
    nr = _split_table(rows, 82, {3: (one_pass + 100, 100), 7: (1, 0)})
    pr, o = _run_mixed(oracle, monkeypatch, nr, waves, 82)
    d, tol = pr["name_digit"], pr["tolerates_unschedulable"] == 1
    r3 = np.flatnonzero((nr["name_digit"] == 3) & (nr["unschedulable"] == 0))
    second = r3[one_pass]  # the lists are in row order: S's entries from here on are the second pass's
    won = o["node"][(d == 3) & ~tol]
    assert (won >= second).any() and (won < second).any()
    assert (nr["unschedulable"][o["node"][(d == 3) & tol]] == 1).any()
    assert (d == 7).sum() > 0 and np.all(o["node"][d == 7] == np.flatnonzero(nr["name_digit"] == 7)[0])
    _assert_cordoned_only_tolerated(nr, pr, o)


def test_block_counts(oracle, monkeypatch):
    # chunk 0 (120 pods), permuted: digits 0 - 4 hold 1, 7, 8, 9 and 15 pods of each kind
    # (a lone pod, a part block, a whole one, one and a rest of 1, one and a rest of 7:
    # the absent pods of a part block must write nothing, neither into the next run's
    # rows nor past the table's end); digit 6, wholly cordoned, 5 of each kind: those that tolerate are covered by U_6,
    # the others are not and take the planes path (level 1), as do 30 pods without a
    # digit: covered, uncovered and planes-path pods side by side. The other chunks cycle.
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    chunk = 120
    assert _table_fits(chunk, 0, 16, 1)
    pr = synth.pods(chunk * _cus(), seed=83)
    pr["tolerates_unschedulable"] = 0
    pr["tolerates_unschedulable"][chunk::5] = 1
    mix = {0: 1, 1: 7, 2: 8, 3: 9, 4: 15, 6: 5}
    dig = np.concatenate([np.full(2 * k, dg) for dg, k in mix.items()] + [np.full(30, -1)])
    tol = np.concatenate([np.repeat([0, 1], [k, k]) for k in mix.values()] + [np.zeros(30, dtype=np.int64)])
    assert len(dig) == chunk and len(tol) == chunk
    perm = np.random.default_rng(83).permutation(chunk)
    dig, tol = dig[perm], tol[perm] == 1
    pr["name_digit"][:chunk] = dig
    pr["tolerates_unschedulable"][:chunk] = tol
    nr = synth.nodes(3000, seed=83)
    nr["unschedulable"][nr["name_digit"] == 6] = 1
    o = oracle.schedule(nr, pr, seed=83)
    with engine_with(nr, seed=83) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)
    s, c = o["score"][:chunk], o["code"][:chunk]
    assert np.all(s[(dig >= 0) & (dig <= 4)] == 10)
    assert np.all(s[(dig == 6) & tol] == 10) and np.all(nr["name_digit"][o["node"][:chunk][(dig == 6) & tol]] == 6)
    assert np.all(s[(dig == 6) & ~tol] == 0) and np.all(c[(dig == 6) & ~tol] == 0)
    # (NodeNumber's Score fails on a pod name without a digit: the cycle's error path)
    assert np.all(s[dig < 0] == 0) and np.all(c[dig < 0] == _lib.CODE_ERROR)
    _assert_cordoned_only_tolerated(nr, pr, o)


def test_zero_hash_is_a_candidate(oracle, monkeypatch):
    # pod ordinal j and row r < 3,000 with tie-break hash exactly 0 (_zero_hash_pods
    # searches j below 2^26 and fails when it finds none); r is the only schedulable row of
    # its digit, so the digit's S tile is r and 191 copies, every lane's maximum for pod j
    # is 0 and so is its row of the table: the final pass must take that 0 as row r's hash
    # at level 11, by the pod's class. The digit's pods that tolerate see the cordoned
    # rows too.
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    seed, n = 84, 3000
    (j, r), = _zero_hash_pods(seed, n, want=1)
    nr = synth.nodes(n, seed=seed)
    nr["unschedulable"] = 0
    dg = int(nr["name_digit"][r])
    nr["unschedulable"][(nr["name_digit"] == dg) & (np.arange(n) != r)] = 1
    pr = synth.pods(_n_pods(), seed=seed, start=1 << 27)
    pr["tolerates_unschedulable"] = np.random.default_rng(seed).random(len(pr)) < 0.2
    k = 37
    pr["ordinal"][k] = j
    pr["name_digit"][k] = dg
    pr["tolerates_unschedulable"][k] = 0
    o = oracle.schedule(nr, pr, seed=seed)
    assert o["node"][k] == r and o["score"][k] == 10 and o["code"][k] == 0
    with engine_with(nr, seed=seed) as e:
        res = e.schedule(pr, MODE_BATCHED)
    assert res["node"][k] == r and res["score"][k] == 10
    assert_same(res, o)
    d, tol = pr["name_digit"], pr["tolerates_unschedulable"] == 1
    assert np.all(o["node"][(d == dg) & ~tol] == r) and ((d == dg) & tol).sum() > 0
    _assert_cordoned_only_tolerated(nr, pr, o)


def _fit_boundary():
    # 16-wave workgroups, one per CU while chunks stay <= 1024 pods: the largest chunk
    # that takes the table form and the next multiple of 8
    lo = max(c for c in range(80, 1025, 8) if _table_fits(c, 0, 16, 1))
    return lo, lo + 8


@pytest.mark.parametrize("side", [0, 1])
def test_fit_boundary(oracle, monkeypatch, side):
    # chunk x CUs pods in one fused device-side cycle (the host-array calls split batches
    # of this size): the last chunk size with the table (all but 2 KiB of a CU's LDS in
    # one workgroup) and the first without, which reduces per wave as before
    import torch

    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    chunk = _fit_boundary()[side]
    assert 104 < chunk <= 1024 and _table_fits(chunk, 0, 16, 1) == (side == 0)
    assert _lds_bytes(chunk, LANE_WORDS if side == 0 else 0) <= LDS_PER_CU
    seed = 85 + side
    nr = synth.nodes(3000, seed=seed)
    pr = _mixed_pods(chunk * _cus(), seed)
    o = oracle.schedule_nunn_omp(nr, pr, seed=seed)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods_d = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    res_d = torch.empty(len(pr) * 24, dtype=torch.uint8, device=dev)
    with engine_with(nr, seed=seed) as e:
        e.select_batch_device(len(pr), pods_d.data_ptr(), res_d.data_ptr(), s.cuda_stream)
        s.synchronize()
    assert_same(res_d.cpu().numpy().view(_lib.RESULT), o)
    assert np.all(o["score"][pr["name_digit"] >= 0] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("node_base", [7, 999_990])
def test_lane_table_node_base(oracle, monkeypatch, node_base):
    # the final pass finds a pod's lists by its sort slot moved back by the table's base;
    # digit 6 wholly cordoned, so its two kinds of pods part ways there
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    nr = synth.nodes(3000, seed=87, start=node_base)
    nr["unschedulable"][nr["name_digit"] == 6] = 1
    pr, o = _run_mixed(oracle, monkeypatch, nr, 16, 87, node_base)
    d, tol = pr["name_digit"], pr["tolerates_unschedulable"] == 1
    assert ((d == 6) & tol).sum() > 0 and ((d == 6) & ~tol).sum() > 0
    assert np.all(o["score"][(d == 6) & ~tol] == 0) and np.all(o["score"][(d == 6) & tol] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o, node_base)
