"""The explain reference (tests/_explain_ref.py) is judged on the CPU before it
judges the GPU: on every case of tests/_explain_cases.py the argmax of its rows'
keys and its counts must equal what the oracle's scheduling calls return, pod by
pod. Struct sizes, the hand KATs of DESIGN.md §2 and the two encoders too."""
import numpy as np
import pytest

import _explain_cases as cases
import _explain_ref as ref
import _nam_required_ref as nref
from minisched_amd import _lib, encode, synth


def oracle_results(oracle, c):
    present, nodes = ref.node_state(c)
    tab = nodes.copy()
    tab["allowed_pods"][~present] = -1  # (the oracle's tombstone)
    ps, kw = c["plugin_set"], dict(seed=c["seed"], node_base=c["node_base"])
    if ps in (0, 1):
        return oracle.schedule(tab, c["pods"], plugin_set=ps, mode=oracle.MODE_BATCHED, **kw)
    if ps == 2:
        return oracle.schedule_na(tab, c["pods"], weights=c["weights"], literal=True, **kw)
    if ps == 3:
        return oracle.schedule_tt(tab, c["pods"], literal=True, **kw)
    return nref.schedule_tombstone(oracle, tab, c["pods"], c["term_sets"], c["req_sets"], weights=c["weights"],
                                   literal=True, **kw)


@pytest.mark.parametrize("ps", range(5))
def test_reference_agrees_with_the_oracle(oracle, ps):
    todo = [c for c in cases.all_cases().values() if c["plugin_set"] == ps]
    assert len(todo) >= len(cases.SIZES) * 4
    for c in todo:
        rows, sums = cases.reference(c)
        o = oracle_results(oracle, c)
        for j in range(len(c["pods"])):
            node, score, code, mask = ref.decode(sums[j])
            want = (int(o["node"][j]), int(o["score"][j]), int(o["code"][j]), int(o["mask"][j]))
            assert (node, score, code, mask) == want, (c["tag"], j)
            # the summary's key is the argmax of the rows, and the oracle's key where it reports one
            assert int(rows["key"][j].max()) == int(sums["best_key"][j]), (c["tag"], j)
            if code == 0 and "key" in o:
                assert int(o["key"][j]) == int(sums["best_key"][j]), (c["tag"], j)
        assert np.array_equal(sums["present"], sums["feasible"] + sums["rejected"].sum(axis=1)), c["tag"]
        scored = rows["key"] != 0
        assert np.array_equal(rows["weighted"].sum(axis=2)[scored], (rows["key"] >> np.uint64(52))[scored]), c["tag"]
        assert not rows["raw"][~scored].any() and not rows["weighted"][~scored].any(), c["tag"]


def test_keys_are_the_oracles_r3(oracle):
    # _explain_ref computes keys in numpy; the oracle's msor_h32 / msor_key pair by pair on three cases
    L = oracle.lib()
    for tag in ("set0 n=65 dead=0% base=33333", "tt F=5", "nam late rescale"):
        c = cases.all_cases()[tag]
        rows, _ = cases.reference(c)
        for j in (0, 13, 39):
            for i in np.nonzero(rows["key"][j])[0][:60]:
                node = c["node_base"] + int(i)
                score = int(rows["weighted"][j, i].sum())
                want = L.msor_key(score, L.msor_h32(c["seed"], int(c["pods"]["ordinal"][j]), node), node)
                assert int(rows["key"][j, i]) == want, (tag, j, i)


def test_least_allocated_is_the_oracles(oracle):
    # _la_cases.la_score (Python integers) against msor_least_requested wherever that cannot overflow
    L = oracle.lib()
    c = cases.all_cases()["la pairs"]
    n = 0
    for x in c["nodes"]:
        for p in c["pods"]:
            cap, req = int(x["alloc_milli_cpu"]), int(x["nonzero_milli_cpu"]) + int(p["nonzero_milli_cpu"])
            if cap < 1 << 56 and req < 1 << 62:
                assert L.msor_least_requested(req, cap) == cases._la_cases.la_score(cap, x["nonzero_milli_cpu"],
                                                                                    p["nonzero_milli_cpu"])
                n += 1
    assert n > 1000


def test_case_coverage():
    # what the family must contain: a (pod, tile) with no present row and one with present rows but
    # none feasible; F = 0..5 exactly; all nine TaintToleration counts; every first-failure status
    T = cases.T
    seen_empty = seen_infeasible = False
    for c in [cases.all_cases()[f"set{ps} n={2 * T + 37} dead=90% base=0"] for ps in range(5)]:
        rows, _ = cases.reference(c)
        st = rows["status"]
        for t0 in range(0, st.shape[1], T):
            tile = st[:, t0:t0 + T]
            seen_empty |= bool((tile == ref.ABSENT).all(axis=1).any())
            some = (tile != ref.ABSENT).any(axis=1) & ~(tile == 0).any(axis=1)
            seen_infeasible |= bool(some.any())
    assert seen_empty and seen_infeasible
    for F in range(6):
        _, sums = cases.reference(cases.all_cases()[f"tt F={F}"])
        assert F in sums["feasible"].tolist() and sums["feasible"].max() > 2 * T
    rows, _ = cases.reference(cases.all_cases()["tt counts 0..8"])
    assert set(np.unique(rows["raw"][0, :, 1][rows["key"][0] != 0]).tolist()) == set(range(9))
    statuses = set()
    for c in cases.all_cases().values():
        statuses |= set(np.unique(cases.reference(c)[0]["status"]).tolist())
    assert statuses == {0, 1, 2, 4, 8, ref.ABSENT}


def test_hand_kats():
    # counts [1, 0] end at [100, 100] under the in-loop hook
    rows, _ = cases.reference(cases.all_cases()["tt [1, 0]"])
    assert rows["raw"][0, :, 1].tolist() == [1, 0] and rows["weighted"][0, :, 1].tolist() == [100, 100]
    # raw [30, 120, 250] -> [33, 40, 100]; the middle node filtered out: [40, 100]
    rows, _ = cases.reference(cases.all_cases()["nam KAT filtered=False"])
    assert rows["raw"][0, :, 1].tolist() == [30, 120, 250] and rows["weighted"][0, :, 1].tolist() == [33, 40, 100]
    assert rows["weighted"][0, :, 0].tolist() == [70, 0, 0]  # NodeNumber under weight 7
    rows, sums = cases.reference(cases.all_cases()["nam KAT filtered=True"])
    assert rows["status"][0].tolist() == [0, 8, 0] and rows["weighted"][0, :, 1].tolist() == [40, 0, 100]
    assert sums["rejected"][0].tolist() == [0, 0, 0, 1]
    # a raw 250 node in the last tile rescales every scored row of the first (weight 2)
    rows, _ = cases.reference(cases.all_cases()["nam late rescale"])
    first = rows[0, :cases.T]
    first = first[first["key"] != 0]
    assert len(first) > 100 and (first["weighted"][:, 1] < 2 * 100 * 100 // 250 + 1).all()


def test_struct_sizes():
    assert _lib.EXPLAIN_ROW.itemsize == 24 and _lib.EXPLAIN_SUMMARY.itemsize == 32
    assert _lib.EXPLAIN_ROW.fields["status"][1] == 16 and _lib.EXPLAIN_SUMMARY.fields["best_key"][1] == 24
    assert "ms_explain" in _lib.SIGNATURES and "ms_explain_device" in _lib.SIGNATURES


def readme_case():
    first, node10, pod1 = synth.readme_scenario()
    return cases.case(0, first, pod1, seed=1, tag="readme")


def test_fit_error_message_on_the_readme_scenario():
    # sched.go:70-140: node0..node8 cordoned, pod1 -> FitError. k8s v1.22 framework/types.go
    # FitError.Error(): "0/%v nodes are available: %v." over the sorted "<count> <reason>" strings,
    # nodeunschedulable.ErrReasonUnschedulable = "node(s) were unschedulable"
    rows, sums = ref.explain(readme_case())
    msg = encode.fit_error_message(sums[0])
    assert msg == "0/9 nodes are available: 9 node(s) were unschedulable."
    assert msg.rstrip(".") == "0/9 nodes are available: 9 node(s) were unschedulable"
    two = np.zeros(1, dtype=_lib.EXPLAIN_SUMMARY)[0]
    two["present"], two["rejected"] = 12, (3, 7, 0, 2)
    assert encode.fit_error_message(two) == ("0/12 nodes are available: 2 node(s) didn't match Pod's node "
                                             "affinity/selector, 3 node(s) were unschedulable, 7 Insufficient cpu, "
                                             "memory or pods.")


def test_explain_annotations():
    names = [f"node{i}" for i in range(9)]
    rows, _ = ref.explain(readme_case())
    filt, score, final = encode.explain_annotations(rows[0], names, 0)
    assert filt == {n: {"NodeUnschedulable": "node(s) were unschedulable"} for n in names}
    assert score == {} and final == {}
    # the KAT cluster: the filtered node has entries up to and including the failing plugin, and no score
    c = cases.all_cases()["nam KAT filtered=True"]
    rows, _ = cases.reference(c)
    filt, score, final = encode.explain_annotations(rows[0], ["a", "b", "c"], 4)
    assert filt["a"] == {"NodeUnschedulable": "passed", "NodeAffinity": "passed"}
    assert filt["b"] == {"NodeUnschedulable": "passed",
                         "NodeAffinity": "node(s) didn't match Pod's node affinity/selector"}
    assert score == {"a": {"NodeNumber": "10", "NodeAffinity": "30"}, "c": {"NodeNumber": "0", "NodeAffinity": "250"}}
    assert final == {"a": {"NodeNumber": "70", "NodeAffinity": "40"}, "c": {"NodeNumber": "0", "NodeAffinity": "100"}}
    # an absent node has no entry; a non-digit pod has filter entries only
    c = cases.all_cases()["set3 n=5 dead=90% base=0"]
    rows, _ = cases.reference(c)
    filt, score, _ = encode.explain_annotations(rows[20], [f"n{i}" for i in range(5)], 3)
    assert set(filt) == {f"n{i}" for i in np.nonzero(rows["status"][20] != ref.ABSENT)[0]} and score == {}
