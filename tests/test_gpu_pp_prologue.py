"""K1 pp's list-form prologue (ms_sweep_pp.hip: plane_classes_ahead, the planes
loaded and sweep_range run only where a class of the chunk needs them) against the
CPU oracle.

What a list-form workgroup does after its sort depends on its own chunk alone: a
chunk in which every pod has a digit whose lists hold a candidate for it loads no
plane, detects no mode and never enters sweep_range, so sweep_lists alone answers
for every pod of it; a chunk with a pod without a digit, a pod that does not
tolerate of a digit with S_d empty, or a pod of a digit with no row at all runs
both. The cases put both kinds of chunk into one launch (those fail for a kernel
that skips the planes in every list-form chunk); the others are parity cases of the
path without planes, where sweep_lists alone decides every pod: few digits, digits of
one row, of two passes, of U tiles alone, short chunks, a chunk of one class. The
geometry is test_gpu_pp_class_runs.py's (MINISCHED_PP_WAVES = 16: chunks of 104
pods; 4: the balanced split's chunks of 104 and 96). Every case compares
node, code, score and plugin mask of every pod, and asserts from the oracle's own
result what it was built to show.
"""
import numpy as np
import pytest

from minisched_amd import _lib, synth
from minisched_amd._lib import MODE_BATCHED
from test_gpu_parity import assert_same, engine_with, need_gpu  # noqa: F401
from test_gpu_pp_class_runs import _cus, _n_pods
from test_gpu_pp_shared_lists import _assert_cordoned_only_tolerated, _mixed_pods, _run_mixed, _split_table

pytestmark = pytest.mark.gpu

WAVES = [16, 4]


def _chunk_range(n, waves, b):
    # pods [lo, hi) of workgroup b (sweep_pp_impl: one round of 16 / waves workgroups per
    # CU, chunks a multiple of 8; 4-wave workgroups take the balanced split, `cb` pods
    # each and 8 more for the first `nx`)
    slots = _cus() * (16 // waves)
    if waves <= 4:
        cb = n // slots // 8 * 8
        nx = -(-(n - cb * slots) // 8)
        assert cb >= 80 and 0 < nx <= slots
        lo = b * cb + min(b, nx) * 8
        return lo, min(n, lo + cb + (8 if b < nx else 0))
    chunk = -(-(-(-n // slots)) // 8) * 8
    assert chunk >= 80
    return b * chunk, min(n, (b + 1) * chunk)


def _digit_pods(n, seed):
    # _mixed_pods with a digit for every pod (its every 13th has none)
    pr = _mixed_pods(n, seed)
    none = pr["name_digit"] < 0
    pr["name_digit"][none] = (np.flatnonzero(none) // 13) % 10
    return pr


def _lists(nr):
    # (S_d, U_d) lengths per digit
    d, u = nr["name_digit"], nr["unschedulable"] == 1
    return [(int(((d == k) & ~u).sum()), int(((d == k) & u).sum())) for k in range(10)]


def _run(oracle, monkeypatch, nr, pr, waves, seed, node_base=0):
    monkeypatch.setenv("MINISCHED_PP_WAVES", str(waves))
    o = oracle.schedule_nunn_omp(nr, pr, seed=seed, node_base=node_base)
    with engine_with(nr, seed=seed, node_base=node_base) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)
    return o


def _assert_no_planes(nr, pr):
    # no chunk can need a plane: every pod has a digit, every digit S and U rows
    assert np.all((pr["name_digit"] >= 0) & (pr["name_digit"] <= 9))
    assert all(s > 0 and u > 0 for s, u in _lists(nr)), _lists(nr)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("layout", ["aligned", "iid"])
def test_no_planes(oracle, monkeypatch, waves, layout):
    # no workgroup loads a plane, on a digit-aligned table and on i.i.d. digits (over-full
    # and misaligned groups, whose mode nobody detects now)
    nr = synth.nodes(3000, seed=81)
    if layout == "iid":
        nr["name_digit"] = np.random.default_rng(81).integers(0, 10, len(nr)).astype(np.uint8)
    pr = _digit_pods(_n_pods(waves=waves), 81)
    _assert_no_planes(nr, pr)
    o = _run(oracle, monkeypatch, nr, pr, waves, 81)
    assert np.all(o["score"] == 10) and np.all(o["code"] == 0)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("rows", [2100, 9630])
def test_no_planes_packed_last_word(oracle, monkeypatch, rows):
    # test_class_runs_packed_last_word's row counts: the 4-wave workgroups' packed last
    # word (Wt) is not loaded either
    nr = synth.nodes(rows, seed=82)
    pr = _digit_pods(_n_pods(waves=4), 82)
    _assert_no_planes(nr, pr)
    o = _run(oracle, monkeypatch, nr, pr, 4, 82)
    assert np.all(o["score"] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("waves", WAVES)
def test_one_workgroup_without_digit(oracle, monkeypatch, waves):
    # the pods without a digit all lie in workgroup 5's chunk: it takes the planes and
    # every other workgroup does not, in one launch
    nr = synth.nodes(3000, seed=83)
    pr = _digit_pods(_n_pods(waves=waves), 83)
    lo, hi = _chunk_range(len(pr), waves, 5)
    other = np.arange(lo + 3, hi, 4)
    pr["name_digit"][other] = -1
    assert all(s > 0 and u > 0 for s, u in _lists(nr))
    o = _run(oracle, monkeypatch, nr, pr, waves, 83)
    has = pr["name_digit"] >= 0
    assert (~has).sum() == len(other) > 20
    # (a name without a digit: NodeNumber's PreScore fails, an error with no score)
    assert np.all(o["score"][~has] == 0) and np.all(o["code"][~has] == _lib.CODE_ERROR)
    assert np.all(o["score"][has] == 10) and np.all(o["code"][has] == 0)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("waves", WAVES)
def test_one_workgroup_with_s_empty(oracle, monkeypatch, waves):
    # every row of digit 2 cordoned (S_2 empty); its pods that do not tolerate all lie
    # in workgroup 7's chunk, which takes them through the planes (score 0 on another
    # digit's row); every other chunk's pods of digit 2 tolerate
    nr = _split_table(3000, 84, {2: (0, 250)})
    pr = _digit_pods(_n_pods(waves=waves), 84)
    lo, hi = _chunk_range(len(pr), waves, 7)
    inside = np.zeros(len(pr), dtype=bool)
    inside[lo:hi] = True
    d2 = pr["name_digit"] == 2
    pr["tolerates_unschedulable"][d2 & ~inside] = 1
    pr["tolerates_unschedulable"][np.flatnonzero(d2 & inside)[::2]] = 0
    o = _run(oracle, monkeypatch, nr, pr, waves, 84)
    tol = pr["tolerates_unschedulable"] == 1
    assert (d2 & ~tol).sum() >= 4 and not np.any(d2 & ~tol & ~inside)
    assert np.all(o["score"][d2 & ~tol] == 0) and np.all(o["code"][d2 & ~tol] == 0)
    assert np.all(o["score"][~(d2 & ~tol)] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("waves", WAVES)
def test_covered_and_uncovered_in_every_chunk(oracle, monkeypatch, waves):
    # S_2 empty, no row of digit 7 at all, and pods without a digit, beside covered
    # classes in every chunk: sweep_range and sweep_lists both run, and the slots combine
    nr = _split_table(3000, 85, {2: (0, 250), 7: (0, 0), 5: (300, 0)})
    pr, o = _run_mixed(oracle, monkeypatch, nr, waves, 85)
    d, tol = pr["name_digit"], pr["tolerates_unschedulable"] == 1
    zero = (d < 0) | (d == 7) | ((d == 2) & ~tol)
    for m in (d < 0, d == 7, (d == 2) & ~tol, (d == 2) & tol):
        assert m.sum() > 0
    assert np.all(o["score"][zero] == 0) and np.all(o["code"][zero] == np.where(d[zero] < 0, _lib.CODE_ERROR, 0))
    assert np.all(o["score"][~zero] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("node_base", [0, 7, 999_990])
def test_first_slot_not_zero(oracle, monkeypatch, waves, node_base):
    # pods of digits 4 and 9 only, so most sort slots of every chunk are empty; at
    # node_base 7 slot and digit part ways (slots 7 and 2)
    nr = synth.nodes(3000, seed=86, start=node_base)
    pr = _digit_pods(_n_pods(waves=waves), 86)
    pr["name_digit"] = np.where(pr["name_digit"] % 2 == 0, 4, 9)
    _assert_no_planes(nr, pr)
    o = _run(oracle, monkeypatch, nr, pr, waves, 86, node_base)
    assert np.all(o["score"] == 10)
    assert np.array_equal(nr["name_digit"][o["node"] - node_base], pr["name_digit"])
    _assert_cordoned_only_tolerated(nr, pr, o, node_base)


@pytest.mark.parametrize("waves", WAVES)
def test_first_class_without_tile(oracle, monkeypatch, waves):
    # the lowest class with pods has no tile (S_0 empty and no pod of digit 0 tolerates), so
    # every chunk takes the planes for it and the lists for the digits after it
    nr = _split_table(3000, 87, {0: (0, 250)})
    pr = _digit_pods(_n_pods(waves=waves), 87)
    d0 = pr["name_digit"] == 0
    pr["tolerates_unschedulable"][d0] = 0
    o = _run(oracle, monkeypatch, nr, pr, waves, 87)
    assert d0.sum() > 0
    assert np.all(o["score"][d0] == 0) and np.all(o["code"][d0] == 0)
    assert np.all(o["score"][~d0] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("waves", WAVES)
def test_first_digit_single_row(oracle, monkeypatch, waves):
    # digit 0 is one schedulable row: one tile, which wave 0 alone holds
    nr = _split_table(3000, 88, {0: (1, 0)})
    pr = _digit_pods(_n_pods(waves=waves), 88)
    assert all(s > 0 for s, u in _lists(nr))
    o = _run(oracle, monkeypatch, nr, pr, waves, 88)
    d0 = pr["name_digit"] == 0
    row = int(np.flatnonzero(nr["name_digit"] == 0)[0])
    assert d0.sum() > 0 and np.all(o["node"][d0] == row)
    assert np.all(o["score"] == 10)


@pytest.mark.parametrize("waves,rows", [(16, 13_500), (4, 3_600)])
def test_first_digit_two_passes(oracle, monkeypatch, waves, rows):
    # S_0 holds more than 4 x waves tiles (test_uneven_digits' shape): two passes, in
    # chunks that go from the scatter's barrier straight to sweep_lists
    nr = _split_table(rows, 89, {0: (4 * waves * 192 + 100, 60)})
    pr = _digit_pods(_n_pods(waves=waves), 89)
    assert all(s > 0 for s, u in _lists(nr)), _lists(nr)
    o = _run(oracle, monkeypatch, nr, pr, waves, 89)
    assert np.all(o["score"] == 10)
    # some pod of digit 0 wins a row of the second pass's tiles (entries past 4 x waves tiles)
    s0 = np.flatnonzero((nr["name_digit"] == 0) & (nr["unschedulable"] == 0))
    late = np.isin(o["node"][pr["name_digit"] == 0], s0[4 * waves * 192:])
    assert late.any() and not late.all()
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("waves", WAVES)
def test_first_digit_tolerating_only(oracle, monkeypatch, waves):
    # every pod of digit 0 tolerates; S_0 is one tile and U_0 two, so the waves after
    # wave 0 hold U tiles alone (ns == 0 in their first pass)
    nr = _split_table(3000, 90, {0: (192, 384)})
    pr = _digit_pods(_n_pods(waves=waves), 90)
    d0 = pr["name_digit"] == 0
    pr["tolerates_unschedulable"][d0] = 1
    assert all(s > 0 for s, u in _lists(nr))
    o = _run(oracle, monkeypatch, nr, pr, waves, 90)
    assert np.all(o["score"] == 10)
    on_u = nr["unschedulable"][o["node"][d0]] == 1
    assert on_u.any() and not on_u.all()
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("last", [1, 65])
def test_short_last_chunk(oracle, monkeypatch, last):
    # 16-wave workgroups (the balanced split of the 4-wave ones leaves no short chunk):
    # the last chunk holds 1 pod, and 65: one more than a wave's lanes
    n = 104 * (_cus() - 1) + last
    nr = synth.nodes(3000, seed=91)
    pr = _digit_pods(n, 91)
    assert _chunk_range(n, 16, _cus() - 1) == (n - last, n)
    o = _run(oracle, monkeypatch, nr, pr, 16, 91)
    assert np.all(o["score"] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("waves", WAVES)
def test_chunk_of_one_class(oracle, monkeypatch, waves):
    # workgroup 3's pods are all of one class (digit 6, not tolerating)
    nr = synth.nodes(3000, seed=92)
    pr = _digit_pods(_n_pods(waves=waves), 92)
    lo, hi = _chunk_range(len(pr), waves, 3)
    pr["name_digit"][lo:hi] = 6
    pr["tolerates_unschedulable"][lo:hi] = 0
    _assert_no_planes(nr, pr)
    o = _run(oracle, monkeypatch, nr, pr, waves, 92)
    assert np.all(o["score"] == 10)
    assert np.all(nr["name_digit"][o["node"][lo:hi]] == 6) and np.all(nr["unschedulable"][o["node"][lo:hi]] == 0)
    _assert_cordoned_only_tolerated(nr, pr, o)


def test_no_planes_output_forms(oracle, monkeypatch):
    # test_no_planes' first case through the three ways out of the kernel: the decoded
    # results with the bind commit, the compact records, and the packed keys
    import torch

    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    n, seed = 3000, 81
    nr = synth.nodes(n, seed=seed)
    pr = _digit_pods(_n_pods(), seed)
    _assert_no_planes(nr, pr)
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
    assert np.all(o["score"] == 10)
