"""K1 pp's list form (ms_sweep_pp.hip: k_build_cand's dense per-class candidate lists and
sweep_lists) against the CPU oracle.

A class-sorted chunk of a launch whose workgroups hold every row sweeps each digit class
over that class's list, kCandTile = 192 entries to a wave and tile, at most 4 tiles per
wave and pass. The cases force run-forming chunks as test_gpu_pp_class_runs.py does
(MINISCHED_PP_WAVES, n_pods = 100 x CUs) and put the lists' lengths at the edges of that
geometry: 0, 1, 191, 192 and 193 entries, one tile more for tolerating pods than for the
others, one entry more than a pass holds (4 x waves x 192), lists rebuilt by flushes on a
live engine, and classes of 1 .. 7 pods, whose only block is partial. Every case compares
node, code, score and plugin mask of every pod.
"""
import numpy as np
import pytest

from minisched_amd import synth
from minisched_amd._lib import MODE_BATCHED
from test_gpu_parity import assert_same, engine_with, need_gpu  # noqa: F401
from test_gpu_pp_class_runs import _cus, _n_pods, _pods

pytestmark = pytest.mark.gpu


def _table(n, seed, counts):
    # n rows whose name_digit column gives digit d exactly counts[d] rows, all of them
    # schedulable (so both of the digit's lists have that length), at random rows; the
    # other digits share what is left and keep synth's unschedulable bits
    nr = synth.nodes(n, seed=seed)
    left = [d for d in range(10) if d not in counts]
    col = np.concatenate([np.full(k, d) for d, k in counts.items()])
    rest = n - len(col)
    col = np.concatenate([col, np.resize(np.array(left), rest)])
    rng = np.random.default_rng(seed)
    nr["name_digit"] = rng.permutation(col).astype(np.uint8)
    nr["unschedulable"][np.isin(nr["name_digit"], list(counts))] = 0
    return nr


def _run(oracle, monkeypatch, nr, waves, seed):
    monkeypatch.setenv("MINISCHED_PP_WAVES", str(waves))
    pr = _pods(_n_pods(waves=waves), seed)
    o = oracle.schedule_nunn_omp(nr, pr, seed=seed)
    with engine_with(nr, seed=seed) as e:
        res = e.schedule(pr, MODE_BATCHED)
    assert_same(res, o)
    return pr, res


EDGES = {0: 0, 1: 1, 2: 191, 3: 192, 4: 193}


@pytest.mark.parametrize("waves", [16, 4])
def test_list_lengths_at_tile_edges(oracle, monkeypatch, waves):
    # lists of 0, 1, 191, 192 and 193 entries: no candidate (per pod, level 1), one row
    # padded to a tile, a tile less one, a whole tile, a tile and one entry. With 16
    # waves most waves hold no tile of the short lists and skip those classes.
    nr = _table(3000, 61, EDGES)
    pr, res = _run(oracle, monkeypatch, nr, waves, 61)
    d = pr["name_digit"]
    assert np.all(res["score"][d == 0] == 0) and np.all(res["score"][(d >= 1) & (d <= 4)] == 10)
    lone = np.flatnonzero(nr["name_digit"] == 1)
    assert np.all(res["node"][d == 1] == lone[0])


@pytest.mark.parametrize("waves", [16, 4])
def test_list_tile_counts_differ_by_toleration(oracle, monkeypatch, waves):
    # one row of the 192-row digit and one of the 193-row digit unschedulable: the
    # lists of the first are 191 and 192 entries, those of the second 192 and 193,
    # one tile for pods that do not tolerate and two for those that do
    nr = _table(3000, 62, EDGES)
    for dg in (3, 4):
        nr["unschedulable"][np.flatnonzero(nr["name_digit"] == dg)[50]] = 1
    _run(oracle, monkeypatch, nr, waves, 62)


@pytest.mark.parametrize("waves,rows,long_", [(16, 26_000, 4 * 16 * 192), (4, 7_000, 4 * 4 * 192)])
def test_list_two_passes(oracle, monkeypatch, waves, rows, long_):
    # a list of one entry more than the waves hold in one pass (a second pass of one
    # tile, taken by wave 0 alone) beside a list that fills the pass exactly
    nr = _table(rows, 63, {3: long_ + 1, 7: long_})
    _run(oracle, monkeypatch, nr, waves, 63)


@pytest.mark.parametrize("max_batch", [1 << 16, 1024])
def test_lists_follow_the_table(oracle, monkeypatch, max_batch):
    # one engine through three flushes; every schedule against the oracle on the table
    # as it then stands. max_batch = 1024: the pod staging grows at the first call and
    # again at the second, larger one, between two builds of the lists.
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    seed, n0, n1 = 64, 3000, 3500
    cur = synth.nodes(n1, seed=seed)
    new = cur[n0:].copy()
    cur["allowed_pods"][n0:] = -1  # not added yet: absent from the oracle's list
    pr = _pods(125 * _cus(), seed)
    small = pr[:_n_pods()]
    rng = np.random.default_rng(seed)
    with engine_with(cur[:n0], seed=seed, cap=n1, max_batch=max_batch) as e:
        assert_same(e.schedule(small, MODE_BATCHED), oracle.schedule(cur, small, seed=seed))
        # cordon every row of digit 4, delete a tenth of the rows, rename 50 rows to
        # other digits, add 500 rows beyond the old end
        cordon = np.flatnonzero(cur["name_digit"][:n0] == 4)
        cur["unschedulable"][cordon] = 1
        e.upsert(cordon, cur[cordon])
        dead = rng.choice(n0, n0 // 10, replace=False)
        e.delete(dead.astype(np.uint32))
        alive = np.setdiff1d(np.arange(n0), dead)
        moved = rng.choice(alive, 50, replace=False)
        cur["name_digit"][moved] = (cur["name_digit"][moved] + 1 + rng.integers(0, 9, 50)) % 10
        e.upsert(moved, cur[moved])
        cur[n0:] = new
        e.upsert(np.arange(n0, n1), cur[n0:])
        cur["allowed_pods"][dead] = -1
        e.flush()
        o = oracle.schedule_nunn_omp(cur, pr, seed=seed)
        res = e.schedule(pr, MODE_BATCHED)
        assert_same(res, o)
        d4 = (pr["name_digit"] == 4) & (pr["tolerates_unschedulable"] == 0)
        assert np.all(res["score"][d4] == 10) and np.any(res["node"][d4] >= n0)
        # un-cordon
        cordon = np.setdiff1d(cordon, dead)
        cur["unschedulable"][cordon] = 0
        e.upsert(cordon, cur[cordon])
        e.flush()
        assert_same(e.schedule(pr, MODE_BATCHED), oracle.schedule_nunn_omp(cur, pr, seed=seed))


def test_list_rest_blocks(oracle, monkeypatch):
    # chunk 0: digit classes of 1, 2, .., 7 and 15 pods (one partial block each; the
    # last a whole block and a partial one), a tolerating class of a single pod, a
    # class of 40 and 20 pods without a digit, permuted; the other chunks cycle
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    chunk = 104
    pr = synth.pods(chunk * _cus(), seed=65)
    pr["tolerates_unschedulable"] = 0
    pr["tolerates_unschedulable"][chunk::5] = 1
    dig = np.repeat(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1]), [1, 2, 3, 4, 5, 6, 7, 15, 40, 1, 20])
    assert len(dig) == chunk
    tol = (dig == 9).astype(np.uint8)
    perm = np.random.default_rng(65).permutation(chunk)
    pr["name_digit"][:chunk] = dig[perm]
    pr["tolerates_unschedulable"][:chunk] = tol[perm]
    nr = synth.nodes(3000, seed=65)
    o = oracle.schedule(nr, pr, seed=65)
    with engine_with(nr, seed=65) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)
    assert np.all(o["score"][:chunk][dig[perm] >= 0] == 10)
