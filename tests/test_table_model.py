"""The node-table model (tests/_table_model.py) on the CPU: its own unit cases,
and the conditions that keep tests/test_gpu_table_churn.py from passing
vacuously, asserted on the scripts themselves with the model and the oracle
alone: every directed step's stated plane, list or column property holds, the
oracle's results differ between consecutive steps of every directed script in
every plugin set (a delta that changes no outcome tests nothing), and every
random script holds each same-ordinal pattern and each kind of operation.
"""
import numpy as np
import pytest

import _table_model as tm
from minisched_amd import _lib


def _rec(**kw):
    r = np.zeros((), dtype=_lib.NODE_REC)
    r["allowed_pods"] = 110
    for k, v in kw.items():
        r[k] = v
    return r


def test_last_delta_wins_and_counters():
    m = tm.TableModel(8, node_base=100)
    a, b = _rec(zone=1), _rec(zone=2)
    m.upsert([103, 103], [a, b])  # U(a) U(b)
    m.upsert([104], [a])
    m.delete([104])  # U D
    m.delete([105])
    m.upsert([105], [b])  # D U(b)
    m.delete([106, 106])  # D D
    m.upsert([107], [a])
    m.delete([107])
    m.upsert([107], [b])  # U(a) D U(b)
    assert (m.present, m.pending) == (3, 11)  # present counts queued deltas, pending every delta
    assert not m.here.any()  # nothing reached the table yet
    m.drain()
    assert (m.present, m.pending) == (3, 0)
    assert m.here.tolist() == [False, False, False, True, False, True, False, True]
    assert m.recs["zone"].tolist() == [0, 0, 0, 2, 0, 2, 0, 2]


def test_expected_read_of_written_rows_and_tombstones():
    m = tm.TableModel(4, node_base=10)
    m.upsert([10, 11], [_rec(name_digit=12, taints=0x12345, unschedulable=7, zone=9, label2=3, pod_count=4),
                        _rec(name_digit=9, req_memory=1 << 40)])
    m.delete([11])
    m.drain()
    t = m.expected_read()
    assert (t["name_digit"][0], t["taints"][0], t["unschedulable"][0], t["zone"][0]) == (0xFF, 0x2345, 1, 9)
    gone = np.zeros((), dtype=_lib.NODE_REC)
    gone["allowed_pods"], gone["name_digit"] = -1, 0xFF
    for r in (1, 2, 3):  # a tombstone and two rows never added read alike: every column cleared
        assert t[r] == gone
    assert np.array_equal(m.oracle_view()["allowed_pods"], [110, -1, -1, -1])


def test_refused_upsert_queues_and_counts_nothing():
    m = tm.TableModel(4, node_base=10)
    with pytest.raises(tm.CapacityError):
        m.upsert([10, 11, 14], [_rec()] * 3)
    with pytest.raises(tm.CapacityError):
        m.delete([12, 9])
    assert (m.present, m.pending) == (0, 0)


def test_binds_drain_and_refuse_absent_rows():
    m = tm.TableModel(4)
    pod = tm.bind_pod(1, huge=True)
    m.upsert([2], [_rec(req_milli_cpu=500, pod_count=1)])
    m.commit(2, pod)  # (drains first)
    assert m.pending == 0 and m.recs["req_milli_cpu"][2] == 500 + int(pod["req_milli_cpu"]) and m.recs["pod_count"][2] == 2
    before = m.recs.copy()
    m.delete([2])
    for o in (2, 3):  # a tombstone, a row never added
        with pytest.raises(tm.AbsentRow):
            m.uncommit(o, pod)
    assert m.pending == 0  # the refused bind drained all the same
    m.upsert([2], [before[2]])
    m.uncommit(2, pod)
    assert (m.recs["req_milli_cpu"][2], m.recs["nonzero_memory"][2], m.recs["pod_count"][2]) == (500, 0, 1)
    cols = [int(pod[k]) for _, k in tm.BIND_COLS]
    assert min(cols) > 0 and len(set(cols)) == 4 and max(cols) >= 1 << 44


N_DIRECTED = len(tm.directed_scripts())


@pytest.mark.parametrize("ps", range(5))
@pytest.mark.parametrize("idx", range(N_DIRECTED))
def test_directed_scripts_state_their_property_and_move_pods(oracle, idx, ps):
    script = tm.directed_scripts()[idx]
    log = tm.walk(script, ps, oracle)
    assert len(log) >= 5
    for k, (st, value, want, form) in enumerate(log):
        assert st.why and st.prop is not None, (script, k)
        assert value == st.expect, (script, k, st.why, value)
        if k:
            assert tm.differs(want, log[k - 1][2]) > 0, f"{script} step {k} ({st.why}) moves no pod in set {ps}"
    assert script.cap <= 2100 and 256 <= script.n_pods <= 400


def test_directed_scripts_cover_what_they_are_for(oracle):
    scripts = tm.directed_scripts()
    pats = set()
    for st, *_ in tm.walk(scripts[0], 0, oracle):
        pats |= set(tm.ordinal_patterns(st, scripts[0].node_base))
        assert all(op[0] != "BADU" or len(op[1]) == 3 for op in st.ops)
    assert {"UU", "UD", "DU", "DD", "UDU"} <= pats
    assert scripts[0].node_base % 10 and scripts[0].node_base % 30
    # the winner of some digit-3 pod is the renamed row itself in the two plane scripts' rename steps
    for s in scripts[1:5]:
        log = tm.walk(s, 0, oracle)
        renamed = int(np.asarray(log[1][0].ops[0][1])[0])
        assert (np.asarray(log[1][2]["node"]) == renamed).any(), s
    # the list script's lengths sit on both sides of the tile edge
    lens = [v for _, v, _, _ in tm.walk(scripts[5], 0, oracle)]
    assert {tm.CAND_TILE + 1, tm.CAND_TILE, tm.CAND_TILE - 1} <= {a for a, _ in lens}
    assert {0, 1, tm.CAND_TILE} <= {b for _, b in lens} and (0, tm.CAND_TILE) in lens


@pytest.mark.parametrize("seed", tm.RANDOM_SEEDS)
def test_random_scripts_hold_every_pattern_and_operation(oracle, seed):
    kinds, pats, muts = set(), set(), 0
    for ps in range(5):
        script = tm.random_script(seed)
        log = tm.walk(script, ps, oracle)
        assert len(log) == tm.RANDOM_STEPS + 1
        moved = sum(tm.differs(log[k][2], log[k - 1][2]) > 0 for k in range(1, len(log)))
        assert moved >= tm.RANDOM_STEPS - 1, (seed, ps, moved)
        if ps:
            continue  # (the ops depend on the rows present alone: the same in every set)
        for st, _, _, form in log:
            kinds |= {op[0] for op in st.ops} | {form}
            pats |= set(tm.ordinal_patterns(st, script.node_base))
            muts += sum(len(op[1]) for op in st.ops if op[0] == "U")
    assert {"UU", "UD", "DU", "DD", "UDU", "U", "D"} <= pats
    assert {"U", "D", "C", "X", "BADU", "host", "compact", "device"} <= kinds
    assert muts > 40 * tm.RANDOM_STEPS
