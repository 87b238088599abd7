"""The NodeAffinity probe inputs of tests/_nam_probe_cases.py, without a GPU:
the Python model equals the C oracle on them (node, code, score, mask), the
oracle's literal loop equals its closed form on their raw lists, and the probes
cover what tests/test_gpu_nam_probes.py is there to pin (every value of F, the
rescales, the anchors, dying tables), counted on the model alone.

The literal loop costs O(rows^2) per POD in the oracle (1.6 s for one 640-row
state), and a state's in-loop lists depend on the class only, not on the digit.
So on every state of every 640-row table the literal loop runs for one digit
per class (rotating with the state) and the closed form for every pod; state 0
of each table runs the literal loop for every pod.
"""
import numpy as np
import pytest

import _nam_probe_cases as pc
import _nam_required_ref as ref

SMALL = ("all_rows", "shards", "host_chunks", "w23_2")


def _weights(name):
    return (23, 2) if name == "w23_2" else pc.W_PROBE


def _same(got, want, tag):
    for k in ("node", "code", "score", "mask"):
        a, b = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        assert np.array_equal(a, b), (tag, k, np.nonzero(a != b)[0][:8].tolist())


def _nodes(name, targets):
    t = pc.table(pc.base_table(name))
    nr = t.with_digits(targets)
    nr["allowed_pods"][np.asarray(t.dead, dtype=np.int64)] = -1
    return t, nr


@pytest.mark.parametrize("name", SMALL)
def test_model_equals_the_oracle_on_640_rows(oracle, name):
    w = _weights(name)
    for s, targets in enumerate(pc.states(name)):
        t, nr = _nodes(name, targets)
        pr = t.pods()
        want = pc.expect(pc.base_table(name), targets, pr, weights=w)
        _same(want, oracle.schedule_nam_ext(nr, pr, t.ts, weights=w, literal=False, seed=pc.SEED), f"{name} {s} closed")
        cls = ref.set_id(pr) * 2 + pr["tolerates_unschedulable"]
        sub = np.nonzero(pr["name_digit"] == (cls + s) % 10)[0] if s else np.arange(len(pr))
        lit = oracle.schedule_nam_ext(nr, pr[sub], t.ts, weights=w, literal=True, seed=pc.SEED)
        _same({k: want[k][sub] for k in ("node", "code", "score", "mask")}, lit, f"{name} {s} literal")


def test_model_equals_the_oracle_on_multi_tile(oracle):
    t = pc.table("multi_tile")
    pr = t.pods()
    st = pc.states("multi_tile")
    for s in (0, 7):
        want = pc.expect("multi_tile", st[s], pr)
        got = oracle.schedule_nam_ext(t.with_digits(st[s]), pr, t.ts, weights=pc.W_PROBE, literal=False, seed=pc.SEED)
        _same(want, got, f"multi_tile {s}")
        # pods whose target is infeasible for their class may be left out on the GPU: a tenth at the most
        assert (~want["hit"]).mean() <= 0.10
    for targets in st + pc.multi_tile_shard_states():
        assert (~pc.expect("multi_tile", targets, pr)["hit"]).mean() <= 0.10


def test_model_equals_the_tombstone_reference_with_required_sets(oracle):
    t = pc.table("required")
    pr = t.pods()
    rejected = 0
    for s, targets in enumerate(pc.states("required")):
        nr = t.with_digits(targets)
        want = pc.expect("required", targets, pr)
        got = ref.schedule_tombstone(oracle, nr, pr, t.ts, t.rq, weights=pc.W_PROBE, seed=pc.SEED, literal=(s == 0))
        _same(want, got, f"required {s}")
        rejected += int((~want["hit"]).sum())
    # the feasible lists differ per class and the anchor moves
    a, b = pc.class_facts("required"), pc.class_facts("all_rows")
    assert sum(1 for k in a if a[k]["anchor"] and b[k]["anchor"] and a[k]["anchor"][0] != b[k]["anchor"][0]) >= 10
    assert rejected >= 100


def test_literal_loop_equals_closed_form_and_model_on_the_raw_lists(oracle):
    for key, c in pc.model("all_rows").items():
        lit = oracle.nam_inloop(c.raw, literal=True)
        assert np.array_equal(lit, oracle.nam_inloop(c.raw, literal=False)), key
        assert np.array_equal(lit, c.F), key
    M = pc.model("multi_tile")
    keys = sorted(M)
    for i in np.random.default_rng(5).choice(len(keys), size=40, replace=False):
        c = M[keys[int(i)]]
        lit = oracle.nam_inloop(c.raw, literal=True)
        assert np.array_equal(lit, oracle.nam_inloop(c.raw, literal=False)), keys[int(i)]
        assert np.array_equal(lit, c.F), keys[int(i)]


def test_layout_facts_the_states_rely_on():
    # every row of all_rows is probed once; multi_tile probes every segment's tile edges
    assert sorted(r for s in pc.states("all_rows") for r in s) == list(range(640))
    mt = {r for s in pc.states("multi_tile") for r in s}
    n = len(pc.table("multi_tile").nodes)
    assert n == 8 * pc.MULTI_TILE_SEG and pc.MULTI_TILE_CUT % 64 != 0
    for r0 in range(0, n, pc.MULTI_TILE_SEG):
        assert {r0, r0 + 1, r0 + 1023, r0 + 1024, r0 + 1087} <= mt
    assert set(range(n - 40, n)) <= mt
    assert len(pc.states("multi_tile")) == 12 and len(pc.states("shards")) == 10
    assert len(pc.states("required")) == 10 and len(pc.states("w23_2")) == 5 and len(pc.states("host_chunks")) == 3
    # host chunks of 700 pods: the 1,320 pods of a state straddle chunks, classes too
    assert len(pc.table("all_rows").pods()) == 1320


def test_coverage_floors():
    pr = pc.probed_F("all_rows")
    F = np.asarray([p[3] for p in pr])
    assert len(set(F.tolist())) >= 95
    assert ((F >= 1) & (F <= 85)).mean() >= 0.25
    family = set(F.tolist())
    for name in ("multi_tile", "shards", "required", "w23_2", "host_chunks"):
        family |= {p[3] for p in pc.probed_F(name)}
    family |= {p[3] for p in pc.probed_F("multi_tile", pc.multi_tile_shard_states())}
    assert family == set(range(101))
    fa, fm = pc.class_facts("all_rows"), pc.class_facts("multi_tile")
    effective = set().union(*(f["effective"] for f in fm.values()), *(f["effective"] for f in fa.values()))
    assert set(range(101, 401)) <= effective
    # anchors of raw < 100 whose F differs from what the row would get as a non-anchor, probed
    # (all_rows probes every row, so every anchor is probed)
    assert sum(1 for f in fa.values() if f["anchor"] and f["anchor"][1] < 100 and f["anchor"][2] != f["anchor"][3]) >= 20
    for facts in (fa, fm):
        assert sum(f["no_rescale"] for f in facts.values()) >= 10
        assert sum(f["dies"] for f in facts.values()) >= 10
        assert sum(f["raw100"] for f in facts.values()) >= 10
        assert sum(f["raw101"] for f in facts.values()) >= 3
