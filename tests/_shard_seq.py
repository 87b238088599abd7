"""Twelve distinct batches through the node-sharded pipeline (tests/test_gpu_sharded.py,
tests/test_gpu_loopback.py): two full rounds of slot reuse at the library's depth of 4 (5
slots), each batch into its own result buffer, with a node delta before batch 4 and another
before batch 9. A sweep that overwrote a slot's keys before the collective read them, a
collective that overwrote what a decode still read, or a sweep on the wrong side of a
delta gives some batch another batch's (or another table's) result.
"""
import numpy as np

from minisched_amd import _lib, synth

N_NODES = 600
SIZES = (96, 520, 131, 257, 333, 100, 419, 512, 205, 388, 147, 461)  # distinct, 96..520
DELTA_BEFORE = (4, 9)


def case(plugin_set, seed):
    """(tables, batches, table_of): the node table before the first delta, after it and after the
    second; the 12 pod batches; the index of the table in force when batch i is submitted."""
    kw = dict(resources=plugin_set == 1, zones=plugin_set == 2, taints=plugin_set == 3)
    nr0 = synth.nodes(N_NODES, seed=seed, **kw)
    nr1 = nr0.copy()
    nr1["unschedulable"][::5] ^= 1  # NodeUnschedulable flips on every 5th node
    nr2 = nr1.copy()
    nr2["name_digit"][::7] = (nr2["name_digit"][::7] + 3) % 10  # NodeNumber digits move
    batches = [synth.pods(n, seed=seed + 1 + i, **kw) for i, n in enumerate(SIZES)]
    table_of = [sum(i >= d for d in DELTA_BEFORE) for i in range(len(SIZES))]
    return (nr0, nr1, nr2), batches, table_of


def _oracle(oracle, nr, pr, plugin_set, seed):
    if plugin_set == _lib.PLUGINS_NU_NN_NA:
        return oracle.schedule_na(nr, pr, seed=seed, literal=False)
    if plugin_set == _lib.PLUGINS_NU_TT_NN:
        return oracle.schedule_tt(nr, pr, seed=seed, literal=False)
    return oracle.schedule(nr, pr, plugin_set=plugin_set, seed=seed)


def _differ(a, b):
    m = min(len(a["node"]), len(b["node"]))
    return any(not np.array_equal(a[k][:m], b[k][:m]) for k in ("node", "code", "score", "mask"))


def expected(oracle, plugin_set, seed):
    """The case with the oracle's result of every batch for the table in force at its submit.
    A stale slot or table must be visible: neighbouring batches' results differ (over their common
    length), and the first batch after each delta differs from its result before the delta."""
    tables, batches, table_of = case(plugin_set, seed)
    want = [_oracle(oracle, tables[table_of[i]], p, plugin_set, seed) for i, p in enumerate(batches)]
    for i in range(1, len(batches)):
        assert _differ(want[i - 1], want[i]), f"batches {i - 1} and {i} have equal results"
    for i in range(5, len(batches)):  # (the batches that share a slot at depth 4)
        assert _differ(want[i - 5], want[i]), f"batches {i - 5} and {i} have equal results"
    for d in DELTA_BEFORE:
        stale = _oracle(oracle, tables[table_of[d] - 1], batches[d], plugin_set, seed)
        assert _differ(stale, want[d]), f"the delta before batch {d} does not change its result"
    return tables, batches, want
