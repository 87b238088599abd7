"""CPU self-check of tests/_la_cases.py, the pair generator behind
tests/test_gpu_la_pairs.py: the C oracle must agree with the Python-integer
model on every pod of every table (so the addressing leaves each pod exactly one
feasible node and the model is the reference's arithmetic), and the generator
must keep its own promises (both sides of every step, decoys in every 16 rows
and every 8 pods, the stated domain). Keeps the GPU tests from going vacuous."""
import numpy as np
import pytest

import _la_cases as lc
from minisched_amd._lib import NODE_REC, POD_REC


@pytest.mark.parametrize("kind", lc.KINDS)
def test_oracle_equals_model(oracle, kind):
    n_probes, tabs = lc.tables(kind, NODE_REC, POD_REC)
    assert n_probes > 20_000 and len(tabs) * lc.PROBES_PER_TABLE >= n_probes
    for t in tabs:
        o = oracle.schedule(t.nodes, t.pods, plugin_set=1, mode=0, seed=t.seed)
        for k_or, want in (("node", t.node), ("code", t.code), ("score", t.score), ("mask", t.mask), ("key", t.key)):
            bad = np.nonzero(o[k_or] != want)[0]
            assert len(bad) == 0, f"{k_or}: oracle {o[k_or][bad[0]]} model {want[bad[0]]}: {lc.describe(t, int(bad[0]))}"
        # sequential: a node is addressed by one pod, so the same results and the model's binds
        o = oracle.schedule(t.nodes, t.pods, plugin_set=1, mode=1, seed=t.seed)
        assert np.array_equal(o["node"], t.node) and np.array_equal(o["score"], t.score)
        a = lc.after_binds(t)
        for k_or, f in (("pod_count", "pod_count"), ("req_cpu", "req_milli_cpu"), ("req_mem", "req_memory"),
                        ("nz_cpu", "nonzero_milli_cpu"), ("nz_mem", "nonzero_memory")):
            assert np.array_equal(getattr(o["cols"], k_or), a[f]), f


@pytest.mark.parametrize("kind", lc.KINDS)
def test_one_feasible_node_per_pod(kind):
    # the addressing itself, pair by pair: pod of probe k fits row probe_row[k] and no other
    _, tabs = lc.tables(kind, NODE_REC, POD_REC)
    for t in tabs[:: max(1, len(tabs) // 3)]:
        free_c = t.nodes["alloc_milli_cpu"] - t.nodes["req_milli_cpu"]
        free_m = t.nodes["alloc_memory"] - t.nodes["req_memory"]
        ok = (t.pods["req_milli_cpu"][:, None] <= free_c[None, :]) & (t.pods["req_memory"][:, None] <= free_m[None, :])
        ok &= (t.nodes["unschedulable"] == 0)[None, :]
        assert np.array_equal(ok.sum(1)[t.probe_pod], np.ones(len(t.probe_pod)))
        assert np.array_equal(ok.argmax(1)[t.probe_pod], t.probe_row)
        decoys = np.setdiff1d(np.arange(len(t.pods)), t.probe_pod)
        assert not ok[decoys].any()
        # the model's filter on the addressed pair and on a neighbour
        for k in (0, len(t.probe_pod) // 2, len(t.probe_pod) - 1):
            r, p = int(t.probe_row[k]), int(t.probe_pod[k])
            assert lc.filter_pair(t.nodes[r], t.pods[p]) == (True, 0)
            if r + 1 < t.M and not t.nodes["unschedulable"][r + 1]:
                assert lc.filter_pair(t.nodes[r + 1], t.pods[p]) == (False, lc.MASK_NRF)


def test_step_points_cover_both_sides():
    caps = [c for c in lc.FAST_CAPS + lc.GENERAL_CAPS + lc.HUGE_CAPS if c >= 200]
    assert len(caps) >= 35
    for cap in caps:
        ds = set(lc.step_points(cap))
        got = {(t[0] - t[1] - t[2]) for t in lc.triples(cap) if t[1] == 0}
        assert ds <= got  # every step point appears with nz = 0
        for k in range(1, 101):
            below = [d for d in ds if d * 100 < k * cap]
            above = [d for d in ds if d * 100 >= k * cap]
            # the last d of step k - 1 and the first d of step k
            assert max(below) * 100 // cap == k - 1 and min(above) * 100 // cap == k, (cap, k)
            assert max(below) + 1 == min(above)
        assert {0, -1, cap} <= ds
        for nzv in ("zero", "mid", "n0", "over"):
            sel = [t for t in lc.triples(cap) if (nzv == "zero" and t[1] == 0) or (nzv == "mid" and t[1] == cap // 3)
                   or (nzv == "n0" and t[2] == 0) or (nzv == "over" and t[1] > cap + 1)]
            assert len(sel) >= {"over": 3, "mid": min(200, cap // 2)}.get(nzv, min(300, cap)), (cap, nzv)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_table_composition(kind):
    n_probes, tabs = lc.tables(kind, NODE_REC, POD_REC)
    lc.check_domain(lc.probes(kind))
    caps = set()
    for t in tabs:
        ac, am = t.nodes["alloc_milli_cpu"], t.nodes["alloc_memory"]
        caps |= set(ac[t.probe_row].tolist())
        probe_max = max(int(ac[t.probe_row].max()), int(am[t.probe_row].max()))
        slow_row = (ac >= lc.K_FAST_CAP) | (am >= lc.K_FAST_CAP)
        huge_row = (ac >= lc.K_HUGE_CAP) | (am >= lc.K_HUGE_CAP)
        slow_pod = (t.pods["nonzero_milli_cpu"] >= lc.K_HUGE_CAP) | (t.pods["nonzero_memory"] >= lc.K_HUGE_CAP)
        windows = lambda v, w: [v[a:a + w].any() for a in range(0, len(v) - w + 1)]
        if kind == "fast":
            assert not slow_row.any() and probe_max < lc.K_FAST_CAP
        if kind == "general":  # a row outside the binary64 range in every 16 rows, none huge
            assert all(windows(slow_row, 16)) and slow_row[::16].all() and not huge_row.any()
        if kind == "huge":
            assert all(windows(huge_row, 16)) and huge_row[::16].all()
        if kind in ("general", "huge"):
            assert t.nodes["unschedulable"][::16].all() and t.nodes["unschedulable"].sum() == len(t.nodes[::16])
        if kind == "slowpods":
            assert not slow_row.any() and all(windows(slow_pod, 8)) and slow_pod[::8].all()
            assert (t.code[::8] == lc.CODE_UNSCHEDULABLE).all()
        assert len(t.probe_row) == lc.PROBES_PER_TABLE and t.M == tabs[0].M and len(t.pods) == len(tabs[0].pods)
    want = set(lc.FAST_CAPS) | (set(lc.GENERAL_CAPS) if kind == "general" else set()) | (
        set(lc.HUGE_CAPS) if kind == "huge" else set())
    assert caps == want
    assert n_probes == len(lc.probes(kind))


def test_walk_points():
    for cap in lc.WALK_CAPS:
        pods, scores, nz = lc.walk(cap, POD_REC, node_digit=3)
        # the node ends over-committed by one; LeastAllocated alone walks 100 .. 0 through every step
        la = scores - np.where(np.arange(len(scores)) % 10 == 3, 10, 0)
        assert nz == cap + 1 and la[0] == 100 and la[-1] == 0 and (np.diff(la) <= 0).all()
        assert cap < 200 or set(la.tolist()) == set(range(101))
        assert (pods["req_milli_cpu"] == 0).all() and (pods["req_memory"] == 0).all()
        assert (pods["nonzero_milli_cpu"][1:] > 0).all() and (pods["nonzero_milli_cpu"] == pods["nonzero_memory"]).all()
