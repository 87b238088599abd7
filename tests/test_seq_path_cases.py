"""CPU self-check of tests/_seq_path_cases.py, the directed contention cases behind
tests/test_gpu_seq_paths.py. Conditions on the inputs, checked with the C oracle
and without a GPU, so that a later edit of a case cannot silently stop reaching
the validator route it is named for: every case reaches its classes, the plateau
holds where it is claimed, the classes do not depend on the tile size, and all
cases together reach every class and every FitError mask route."""
import pytest

import _seq_path_cases as sp
from minisched_amd._lib import NODE_REC, POD_REC

NAMES = [c.name for c in sp.CASES]


def model(oracle, case, tile_rows, simulate=True):
    nodes, gone, pods, n_fill, o = sp.prepared(case, oracle, NODE_REC, POD_REC, tile_rows)
    return sp.run_model(case, nodes, pods, o, tile_rows, simulate=simulate), (nodes, gone, pods, n_fill, o)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_classes(oracle, name):
    case = sp.CASE[name]
    (cls, sim), (nodes, gone, pods, n_fill, o) = model(oracle, case, 80)
    for w in case.want:
        assert cls[w] >= 1, (name, w, dict(cls))
    # only hot rows ever win, and the directed pods are not all of one kind
    won = o["node"][o["code"] == sp.CODE_SUCCESS]
    assert len(won) and set(won.tolist()) <= set(case.hot(80))
    assert (o["code"][:n_fill] == sp.CODE_UNSCHEDULABLE).all()
    if case.nodigit:
        assert (o["code"] == sp.CODE_ERROR).sum() >= 5
    if case.tol:  # both masks among the FitErrors: NU|NRF without the toleration, NRF with it
        m = o["mask"][n_fill:][o["code"][n_fill:] == sp.CODE_UNSCHEDULABLE]
        assert {sp.MASK_NRF, sp.MASK_NU | sp.MASK_NRF} <= set(m.tolist()), set(m.tolist())
    if case.plateau:
        sp.plateau_ok(case, nodes, pods, o)
    # the restated rounds (simulate_batch agreed with the oracle pod by pod inside run_model)
    # reach the routes the case is named for, and send the FitErrors the same way
    if case.bounds:
        assert sim["pods"] == len(pods)
        for w in case.want:
            k = {"walk": "max_walk", "ext": "recompute", "fast": "pods"}.get(w, w)
            assert sim[k] >= 1, (name, w, dict(sim))
        for r in sp.FIT_ROUTES:
            assert sim[r] == cls[r], (r, dict(sim), dict(cls))


def test_structural_classes_are_no_lower_bound(oracle):
    # a pod is resolved against the state at the start of its round: it does not see the binds
    # of the pods between the round's start and itself, so fewer pods scan than have every
    # certified rank bound by an earlier pod (why the GPU test asserts the rounds' counts)
    (cls, sim), _ = model(oracle, sp.CASE["spread8"], 80)
    assert (cls["scan"], sim["scan"]) == (33, 27)
    (cls, sim), _ = model(oracle, sp.CASE["block6_hi"], 80)
    assert (cls["fast"], cls["scan"], cls["resweep"]) == (6, 58, 58) == (6, sim["scan"], sim["resweep"])


@pytest.mark.parametrize("name", NAMES)
def test_classes_do_not_depend_on_the_tile_size(oracle, name):
    case = sp.CASE[name]
    ref = None
    for tr in sp.TILE_ROWS:
        (cls, sim), _ = model(oracle, case, tr, simulate=case.bounds)
        if case.by_tile:  # other rows at every size (other tie-breaks): its classes are reached at each
            for w in case.want:
                assert cls[w] >= 1 and sim[w] >= 1, (name, tr, w)
            continue
        got = (dict(cls), dict(sim))
        ref = ref or got
        assert got == ref, (name, tr, got, ref)


def test_all_classes_and_routes_are_reached(oracle):
    total, sims = sp.Counts(), sp.Counts()
    for case in sp.CASES:
        if not case.bounds:
            continue
        (cls, sim), _ = model(oracle, case, 80)
        for k, v in cls.items():
            total[k] += v
        for k, v in sim.items():
            sims[k] += v
    for k in sp.CLASSES + sp.FIT_ROUTES + ("resweep",):
        assert total[k] >= 1, (k, dict(total))
    for k in ("slow", "scan", "resweep", "recompute") + sp.FIT_ROUTES:
        assert sims[k] >= 1, (k, dict(sims))


def test_geometry_promises():
    for case in sp.CASES:
        for tr in sp.TILE_ROWS:
            rows = sorted(case.hot(tr))
            tiles = [r // tr for r in rows]
            blocks = {}
            for r in rows:
                blocks.setdefault(r // 16, []).append(r)
            for b in blocks.values():  # an aligned 16-row block straddles no tile
                assert len({r // tr for r in b}) == 1
            heads = sorted(blocks)
            assert all((b - a) * 16 >= 256 + 16 for a, b in zip(heads, heads[1:])), (case.name, tr)
            assert len(set(tiles)) == len(blocks)
    hi = sp.CASE["block6_hi"].hot(80)
    assert all(r // tr >= 64 for r in hi for tr in sp.TILE_ROWS)
    last = sp.CASE["block6_last_tile_room3"].hot(80)
    assert all(r // tr == (sp.N_NODES - 1) // tr and sp.N_NODES % tr for r in last for tr in sp.TILE_ROWS)
    for tr in sp.TILE_ROWS:
        a, b = sorted({r // tr for r in sp.CASE["blocks_same_lane"].hot(tr)})
        assert b == a + 64
        a, b = sorted({r // tr for r in sp.CASE["blocks_two_lanes"].hot(tr)})
        assert a % 64 != b % 64
    # the filler reaches the full-size batches, the directed pods fill whole ones
    assert sp.batches(sp.WARM_PODS + 256)[-3:] == [(4032, 64), (4096, 128), (4224, 128)]
    assert sp.tile_rows_for(sp.N_NODES, 256) == 80 and sp.tile_rows_for(50_000, 256) == 208


def test_many_walkers_in_one_round(oracle):
    # the 16-pod passes of walk_top4: some round of the case re-resolves more than 16 pods
    case = sp.CASE["spread40_many_walkers"]
    (cls, sim), _ = model(oracle, case, 80)
    assert sim["max_walk"] > 16, dict(sim)
