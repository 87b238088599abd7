"""The 12-batch sequence of tests/_shard_seq.py can see a stale slot or table: checked
on the CPU for every plugin set the GPU tests run it with."""
import pytest

import _shard_seq


@pytest.mark.parametrize("plugin_set", [0, 1, 2, 3])
def test_shard_sequence_results_differ(oracle, plugin_set):
    tables, batches, want = _shard_seq.expected(oracle, plugin_set, 900 + plugin_set)
    assert len(batches) == 12 and len({len(b) for b in batches}) == 12
    assert all(96 <= len(b) <= 520 for b in batches)
    assert len(tables) == 3 and all(len(t) == _shard_seq.N_NODES for t in tables)
    assert [len(w["node"]) for w in want] == [len(b) for b in batches]
