"""K1 pp's list form with one run of tiles per name digit shared by both tolerations
(ms_sweep_pp.hip: k_build_cand's S_d and U_d lists, sweep_lists) against the CPU oracle.

For a digit d, S_d lists the present schedulable rows whose name ends in d and U_d the
present cordoned ones, S_d's tiles then U_d's, each padded to whole tiles of 192 entries.
A wave loads its tiles of the digit once (tiles wave, wave + W, .., 4 per pass), sweeps
the pods that do not tolerate node.kubernetes.io/unschedulable through its S tiles and
the pods that do through all of them. A chunk's pods are sorted digit by digit, the
tolerating ones last. The cases force list-form chunks as test_gpu_pp_cand_lists.py does
(MINISCHED_PP_WAVES, n_pods = 100 x CUs) and put the S / U boundary, the lists' lengths
and the toleration runs at the edges of that geometry. Every case compares node, code,
score and plugin mask of every pod, and asserts from the oracle's own result what it was
built to show.
"""
import numpy as np
import pytest

from minisched_amd import synth
from minisched_amd._lib import MODE_BATCHED
from test_gpu_parity import assert_same, engine_with, need_gpu  # noqa: F401
from test_gpu_pp_cand_lists import _table
from test_gpu_pp_class_runs import _cus, _n_pods, _pods

pytestmark = pytest.mark.gpu


def _split_table(n, seed, lists):
    # n rows in which digit d has exactly lists[d] = (S, U) schedulable and cordoned rows,
    # at random rows; the other digits share what is left and keep synth's cordons
    nr = _table(n, seed, {d: s + u for d, (s, u) in lists.items()})
    rng = np.random.default_rng(seed + 1000)
    for d, (s, u) in lists.items():
        rows = np.flatnonzero(nr["name_digit"] == d)
        assert len(rows) == s + u
        nr["unschedulable"][rng.choice(rows, u, replace=False)] = 1
    return nr


def _mixed_pods(n, seed):
    # _pods lets every fifth pod tolerate: every pod of digits 0 and 5 and no other (which
    # is why test_gpu_pp_cand_lists._run, built on it, is not used here). A digit needs
    # pods of both kinds, so a fifth of the pods of every digit tolerate
    pr = _pods(n, seed)
    pr["tolerates_unschedulable"] = np.random.default_rng(seed + 2000).random(n) < 0.2
    return pr


def _run_mixed(oracle, monkeypatch, nr, waves, seed, node_base=0):
    monkeypatch.setenv("MINISCHED_PP_WAVES", str(waves))
    pr = _mixed_pods(_n_pods(waves=waves), seed)
    o = oracle.schedule_nunn_omp(nr, pr, seed=seed, node_base=node_base)
    with engine_with(nr, seed=seed, node_base=node_base) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)
    return pr, o


def _cordoned_winners(nr, pr, o, node_base=0):
    # winners on cordoned rows, among the pods that tolerate and among those that do not
    ok = o["code"] == 0
    on = np.zeros(len(pr), dtype=bool)
    on[ok] = nr["unschedulable"][o["node"][ok] - node_base] == 1
    tol = pr["tolerates_unschedulable"] == 1
    return int((on & tol).sum()), int((on & ~tol).sum())


def _assert_cordoned_only_tolerated(nr, pr, o, node_base=0):
    t, f = _cordoned_winners(nr, pr, o, node_base)
    assert t > 0 and f == 0, (t, f)


@pytest.mark.parametrize("waves", [16, 4])
def test_s_empty_and_u_empty(oracle, monkeypatch, waves):
    # digit 2: every row cordoned (S empty, U 250 rows): its pods that do not tolerate
    # find no list and score 0 through the planes (level 1), its tolerating pods score
    # 10 on a cordoned row. Digit 5: no row cordoned (U empty): both kinds of its pods
    # see the same tiles.
    nr = _split_table(3000, 71, {2: (0, 250), 5: (300, 0)})
    pr, o = _run_mixed(oracle, monkeypatch, nr, waves, 71)
    d, tol = pr["name_digit"], pr["tolerates_unschedulable"] == 1
    for dg in (2, 5):
        assert ((d == dg) & ~tol).sum() > 0 and ((d == dg) & tol).sum() > 0
    assert np.all(o["score"][(d == 2) & ~tol] == 0) and np.all(o["code"][(d == 2) & ~tol] == 0)
    assert np.all(o["score"][(d == 2) & tol] == 10)
    assert np.all(nr["name_digit"][o["node"][(d == 2) & tol]] == 2)
    assert np.all(o["score"][d == 5] == 10)
    assert np.all(nr["unschedulable"][o["node"][d == 5]] == 0)
    _assert_cordoned_only_tolerated(nr, pr, o)


# (S, U) per digit. U lengths 0, 1, 191, 192 and 193. Where the S / U boundary falls (a
# wave holds tiles w, w + W, ..; ns of its nt tiles are S tiles):
#   W = 4, digit 0: 5 S tiles and 2 U tiles: the first U tile in the middle of a round of
#     the dealing, inside one wave's tiles (waves 1 and 2 hold an S tile and then a U tile,
#     0 < ns < nt; wave 0 holds S tiles only, ns = nt; wave 3 one S tile);
#   W = 4, digit 1: S fills W tiles exactly, so the first U tile starts a round: wave 0's
#     second tile (0 < ns < nt) while waves 1 - 3 stop at their S tile;
#   W = 16, digit 1: the same with 16 S tiles and 2 U tiles (waves 0 and 1: 0 < ns < nt),
#     which is also the only place where one wave holds both kinds at W = 16: a digit needs
#     more than 16 tiles for that, hence 4,600 rows here where the other cases have 3,000;
#   W = 16, digit 0: 2 S tiles and 1 U tile: the boundary between two waves (wave 2 holds
#     a U tile only, ns = 0 < nt);
#   digits 2 - 4, both W: one or two S tiles and one U tile or none, every tile in a wave
#     of its own.
EDGE_LISTS = {
    4: (3000, {0: (5 * 192, 193), 1: (4 * 192, 1), 2: (100, 191), 3: (192, 192), 4: (193, 0)}),
    16: (4600, {0: (193, 1), 1: (16 * 192, 193), 2: (100, 191), 3: (192, 192), 4: (193, 0)}),
}


@pytest.mark.parametrize("waves", [16, 4])
def test_u_lengths_at_tile_edges(oracle, monkeypatch, waves):
    rows, lists = EDGE_LISTS[waves]
    nr = _split_table(rows, 72, lists)
    pr, res = _run_mixed(oracle, monkeypatch, nr, waves, 72)
    d = pr["name_digit"]
    assert np.all(res["score"][(d >= 0) & (d <= 4)] == 10)
    _assert_cordoned_only_tolerated(nr, pr, res)
    # per digit with a U list: some tolerating pod of the digit wins one of its rows
    tol = pr["tolerates_unschedulable"] == 1
    for dg, (s, u) in lists.items():
        won = nr["unschedulable"][res["node"][(d == dg) & tol]] == 1
        assert not (u == 0 and won.any())
        if u >= 191:
            assert won.any(), dg


@pytest.mark.parametrize("waves,rows", [(16, 26_000), (4, 7_000)])
def test_u_tile_alone_in_second_pass(oracle, monkeypatch, waves, rows):
    # S fills one pass exactly (4 x waves tiles) and U holds one row: the second pass
    # holds U's tile only, wave 0 alone takes it, and the pods that do not tolerate skip
    # it. The cordoned row is one that a tolerating pod wins (found by the oracle on a
    # few of those pods with every row of the digit still schedulable).
    long_ = 4 * waves * 192
    nr = _table(rows, 73, {3: long_ + 1})
    monkeypatch.setenv("MINISCHED_PP_WAVES", str(waves))
    pr = _mixed_pods(_n_pods(waves=waves), 73)
    few = np.flatnonzero((pr["name_digit"] == 3) & (pr["tolerates_unschedulable"] == 1))[:4]
    row = int(oracle.schedule_nunn_omp(nr, pr[few], seed=73)["node"][0])
    assert nr["name_digit"][row] == 3
    nr["unschedulable"][row] = 1
    o = oracle.schedule_nunn_omp(nr, pr, seed=73)
    with engine_with(nr, seed=73) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)
    assert o["node"][few[0]] == row
    _assert_cordoned_only_tolerated(nr, pr, o)


def test_chunk_mixing_tolerations(oracle, monkeypatch):
    # chunk 0, per digit (pods that do not tolerate, pods that do): tolerating only,
    # not tolerating only, 5 + 6 (an 8-pod block of the digit's run straddles the
    # boundary), then runs of 1 .. 7 of each kind, and 30 pods without a digit,
    # permuted; the other chunks cycle
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    chunk = 104
    pr = synth.pods(chunk * _cus(), seed=74)
    pr["tolerates_unschedulable"] = 0
    pr["tolerates_unschedulable"][chunk::5] = 1
    mix = {0: (0, 3), 1: (4, 0), 2: (5, 6)}
    mix.update({2 + k: (k, 8 - k) for k in range(1, 8)})
    dig = np.concatenate([np.full(a + b, dg) for dg, (a, b) in mix.items()] + [np.full(30, -1)])
    tol = np.concatenate([np.repeat([0, 1], [a, b]) for a, b in mix.values()] + [np.zeros(30, dtype=np.int64)])
    assert len(dig) == chunk and len(tol) == chunk
    perm = np.random.default_rng(74).permutation(chunk)
    pr["name_digit"][:chunk] = dig[perm]
    pr["tolerates_unschedulable"][:chunk] = tol[perm]
    nr = synth.nodes(3000, seed=74)
    o = oracle.schedule(nr, pr, seed=74)
    with engine_with(nr, seed=74) as e:
        assert_same(e.schedule(pr, MODE_BATCHED), o)
    assert np.all(o["score"][:chunk][dig[perm] >= 0] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o)


@pytest.mark.parametrize("node_base", [7, 999_990])
def test_shared_lists_node_base(oracle, monkeypatch, node_base):
    # the sort key follows the fixed slot (digit - node_base mod 10), the lists follow
    # the digit; one digit wholly cordoned, so its two kinds of pods part ways
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    nr = synth.nodes(3000, seed=75, start=node_base)
    nr["unschedulable"][nr["name_digit"] == 6] = 1
    pr, o = _run_mixed(oracle, monkeypatch, nr, 16, 75, node_base)
    d, tol = pr["name_digit"], pr["tolerates_unschedulable"] == 1
    assert np.all(o["score"][(d == 6) & ~tol] == 0) and np.all(o["score"][(d == 6) & tol] == 10)
    _assert_cordoned_only_tolerated(nr, pr, o, node_base)


def test_cordon_and_uncordon_live(oracle, monkeypatch):
    # one engine through three flushes that move rows between a digit's S and U lists:
    # half of digit 4 and all of digit 6 cordoned; digit 6 back and the rest of digit 4
    # cordoned; everything schedulable. Tolerating pods in every schedule.
    monkeypatch.setenv("MINISCHED_PP_WAVES", "16")
    seed, n = 76, 3000
    cur = synth.nodes(n, seed=seed)
    pr = _mixed_pods(_n_pods(), seed)
    d, tol = pr["name_digit"], pr["tolerates_unschedulable"] == 1
    r4, r6 = np.flatnonzero(cur["name_digit"] == 4), np.flatnonzero(cur["name_digit"] == 6)

    def step(e, *changes):
        for rows, value in changes:
            cur["unschedulable"][rows] = value
            e.upsert(rows, cur[rows])
        e.flush()
        o = oracle.schedule(cur, pr, seed=seed)
        assert_same(e.schedule(pr, MODE_BATCHED), o)
        return o

    with engine_with(cur, seed=seed) as e:
        o = oracle.schedule(cur, pr, seed=seed)
        assert_same(e.schedule(pr, MODE_BATCHED), o)
        _assert_cordoned_only_tolerated(cur, pr, o)
        o = step(e, (r4[::2], 1), (r6, 1))
        assert np.all(o["score"][(d == 6) & ~tol] == 0) and np.all(o["score"][(d == 6) & tol] == 10)
        assert np.all(o["score"][d == 4] == 10)
        _assert_cordoned_only_tolerated(cur, pr, o)
        o = step(e, (r6, 0), (r4, 1))
        assert np.all(o["score"][(d == 4) & ~tol] == 0) and np.all(o["score"][(d == 4) & tol] == 10)
        assert np.all(o["score"][d == 6] == 10)
        _assert_cordoned_only_tolerated(cur, pr, o)
        o = step(e, (np.arange(n), 0))
        assert _cordoned_winners(cur, pr, o) == (0, 0) and np.all(o["score"][d >= 0] == 10)
