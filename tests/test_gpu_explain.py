"""Engine.explain on the GPU against tests/_explain_ref.py (judged on the CPU by
tests/test_explain_ref.py): every row's status, raw, weighted and key and every
summary field, element for element, on the cases of tests/_explain_cases.py;
then the invariants of the call (windows, summary only, argmax, no side effect,
stream ordering, regrow, refusals)."""
import numpy as np
import pytest

import _explain_cases as cases
import _explain_ref as ref
from minisched_amd import _lib, synth
from minisched_amd._lib import MODE_BATCHED, Engine

pytestmark = pytest.mark.gpu
T = cases.T


def engine_for(c, max_nodes=None):
    """A fresh engine holding the case's table (the dead rows upserted, then deleted)."""
    e = Engine(max_nodes=max_nodes or c["max_nodes"], plugin_set=c["plugin_set"], node_base=c["node_base"],
               seed=c["seed"], score_weights=c["weights"] if c["plugin_set"] in (2, 4) else (0, 0))
    e.upsert(c["node_base"] + np.arange(len(c["nodes"])), c["nodes"])
    if len(c["dead"]):
        e.delete(c["node_base"] + c["dead"])
    if c["plugin_set"] == 4:
        e.nam_term_sets_ext(c["term_sets"])
        e.nam_required_sets(c["req_sets"])
    return e


@pytest.mark.parametrize("ps", range(5))
def test_rows_and_summaries(ps):
    todo = [c for c in cases.all_cases().values() if c["plugin_set"] == ps]
    assert len(todo) >= len(cases.SIZES) * len(cases.TOMBSTONES) * len(cases.NODE_BASES)
    for c in todo:
        want_rows, want_sums = cases.reference(c)
        with engine_for(c) as e:
            rows, sums = e.explain(c["pods"])
        ref.same(rows, sums, want_rows, want_sums, c["tag"])


WINDOW_CASES = [f"set0 n={2 * T + 37} dead=0% base=33333", "la pairs", "na anchor", "tt F=5", "tt F=2",
                "nam late rescale", f"set4 n={2 * T + 37} dead=90% base=33333"]


@pytest.mark.parametrize("tag", WINDOW_CASES)
def test_window_invariance_and_summary_only(tag):
    # the rows of a window are the slice of the whole-table rows, wherever the anchor, the rescaling
    # nodes and the first / last feasible rows lie relative to it; the summaries never depend on it
    c = cases.all_cases()[tag]
    want_rows, want_sums = cases.reference(c)
    n = c["max_nodes"]
    windows = [(0, n), (5, 6), (n - 1, n), (min(3, n - 1), min(T + 9, n)), (min(T + 3, n - 1), min(2 * T + 1, n)),
               (min(T, n - 1), n), (0, min(T, n)), (min(2 * T, n - 1), n), (7, 7)]
    with engine_for(c) as e:
        for a, b in windows:
            rows, sums = e.explain(c["pods"], first=c["node_base"] + a, n_nodes=b - a)
            assert rows.shape == (len(c["pods"]), b - a)
            ref.same(rows, sums, want_rows[:, a:b], want_sums, f"{tag} window [{a}, {b})")
        none, sums = e.explain(c["pods"], rows=False)
        assert none is None
        ref.same(want_rows, sums, want_rows, want_sums, f"{tag} summary only")
        rows, none = e.explain(c["pods"], first=c["node_base"] + 3, n_nodes=min(n - 3, T), summaries=False)
        assert none is None
        ref.same(rows, None, want_rows[:, 3:3 + min(n - 3, T)], None, f"{tag} rows only")


@pytest.mark.parametrize("tag", ["set0 n=65 dead=0% base=0", "la pairs", "na anchor", "tt F=5",
                                 f"set3 n={2 * T + 37} dead=0% base=0", "nam late rescale",
                                 f"set4 n={T + 1} dead=0% base=33333"])
def test_argmax_is_the_scheduling_result_and_nothing_is_committed(tag):
    # best_key and the argmax of the whole-table rows decode to Engine.schedule's node and score on a
    # fresh equal engine; schedule / explain / schedule returns identical results and leaves the table as it was
    c = cases.all_cases()[tag]
    pods = c["pods"]
    with engine_for(c) as e:
        r0 = e.schedule(pods, MODE_BATCHED)
    with engine_for(c) as e:
        table0 = e.read(c["node_base"], c["max_nodes"])
        rows, sums = e.explain(pods)
        table1 = e.read(c["node_base"], c["max_nodes"])
        r1 = e.schedule(pods, MODE_BATCHED)
        rows2, sums2 = e.explain(pods)
    assert table0.tobytes() == table1.tobytes()
    assert r0.tobytes() == r1.tobytes()
    for j in range(len(pods)):
        node, score, code, mask = ref.decode(sums[j])
        assert (node, score, code, mask) == (r0["node"][j], r0["score"][j], r0["code"][j], r0["plugin_mask"][j]), (tag, j)
        assert int(rows["key"][j].max()) == int(sums["best_key"][j])
        if code == 0:
            i = int(rows["key"][j].argmax())
            assert c["node_base"] + i == node and int(rows["weighted"][j, i].sum()) == score
    if c["plugin_set"] != 1:  # (the resource-aware set's binds change the table the second explain sees)
        assert rows.tobytes() == rows2.tobytes() and sums.tobytes() == sums2.tobytes()
    assert np.array_equal(sums["present"], sums["feasible"] + sums["rejected"].sum(axis=1))


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


@pytest.mark.parametrize("ps", [2, 1])
def test_stream_ordering(ps):
    # an upsert followed by explain_device on a caller stream with no host synchronise sees the upsert;
    # then the mixed NULL / caller-stream sequence of test_stream_ordering_mixed_null_and_caller_stream
    # with explain as the middle call: select (caller), explain (context), select (caller), ...
    import torch

    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    n, seed = 2 * T + 37, 61
    nr = synth.nodes(n, seed=seed, zones=ps == 2, resources=ps == 1)
    later = synth.nodes(n, seed=seed + 1, zones=ps == 2, resources=ps == 1)
    pods = cases.base_pods(ps, seed)
    c0 = cases.case(ps, nr, pods, seed=seed)
    c1 = cases.case(ps, later, pods, seed=seed)
    rows_d = torch.zeros(len(pods) * n * 24, dtype=torch.uint8, device="cuda:0")
    sums_d = torch.zeros(len(pods) * 32, dtype=torch.uint8, device="cuda:0")
    res_d = [torch.zeros(len(pods) * 24, dtype=torch.uint8, device="cuda:0") for _ in range(4)]
    rows_k = [torch.zeros(len(pods) * n * 24, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    pods_d = _dev(pods)
    with engine_for(c0) as e:
        torch.cuda.synchronize()
        e.upsert(np.arange(n), later)
        e.explain_device(len(pods), pods_d.data_ptr(), 0, n, rows_d.data_ptr(), sums_d.data_ptr(), s.cuda_stream)
        for k in range(4):
            e.select_batch_device(len(pods), pods_d.data_ptr(), res_d[k].data_ptr(), s.cuda_stream)
            if k < 2:
                e.explain_device(len(pods), pods_d.data_ptr(), 0, n, rows_k[k].data_ptr(), 0, None)
        e.read(0, 1)  # context stream: after every call on either stream
        s.synchronize()
    want_rows, want_sums = ref.explain(c1)
    got = rows_d.cpu().numpy().view(_lib.EXPLAIN_ROW).reshape(len(pods), n)
    ref.same(got, sums_d.cpu().numpy().view(_lib.EXPLAIN_SUMMARY), want_rows, want_sums, "after the upsert")
    for k in range(2):
        ref.same(rows_k[k].cpu().numpy().view(_lib.EXPLAIN_ROW).reshape(len(pods), n), None, want_rows, None, f"mixed {k}")
    for k in range(4):
        r = res_d[k].cpu().numpy().view(_lib.RESULT)
        for j in range(len(pods)):
            assert ref.decode(want_sums[j]) == (r["node"][j], r["score"][j], r["code"][j], r["plugin_mask"][j]), (k, j)


def test_regrow():
    # 1 pod, then 256, then a wider window in one live context: the scratch grows twice
    c = cases.all_cases()["nam late rescale"]
    many = np.concatenate([c["pods"]] * 7)[:256].copy()
    many["ordinal"] = np.arange(256)
    big = dict(c, pods=many)
    want_rows, want_sums = ref.explain(big)
    n = c["max_nodes"]
    with engine_for(c, max_nodes=4 * T) as e:
        rows, sums = e.explain(many[:1], n_nodes=T)
        ref.same(rows, sums, want_rows[:1, :T], want_sums[:1], "1 pod")
        rows, sums = e.explain(many, n_nodes=T)
        ref.same(rows, sums, want_rows[:, :T], want_sums, "256 pods")
        rows, sums = e.explain(many)  # the whole range: past the rows ever upserted
        ref.same(rows[:, :n], sums, want_rows, want_sums, "wider window")
        assert (rows["status"][:, n:] == ref.ABSENT).all() and not rows["key"][:, n:].any()


def test_refusals():
    c = cases.all_cases()["set0 n=65 dead=0% base=33333"]
    pods = np.concatenate([c["pods"]] * 7)[:257]
    with engine_for(c) as e:
        with pytest.raises(_lib.MSError) as x:
            e.explain(pods)
        assert x.value.code == _lib.MS_E_INVAL
        for first, k in ((c["node_base"] + 1, 65), (c["node_base"] - 1, 2), (0, 1)):
            with pytest.raises(_lib.MSError) as x:
                e.explain(pods[:3], first=first, n_nodes=k)
            assert x.value.code == _lib.MS_E_CAPACITY
        with pytest.raises(_lib.MSError) as x:
            e.explain(pods[:3], rows=False, summaries=False)
        assert x.value.code == _lib.MS_E_INVAL
        rows, sums = e.explain(pods[:0])  # no pods: MS_OK
        assert rows.shape == (0, 65) and len(sums) == 0
        rows, sums = e.explain(pods[:256])  # the most pods a call takes
        assert rows.shape == (256, 65)
