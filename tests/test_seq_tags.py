"""The chunk sizes of test_gpu_parity.test_chunked_warm_runs against the restated tag
sequence (tests/_seq_tags.py), on the CPU: which tag a batch expects in the pod slots
its run has not swept yet, and which tag an earlier chunk left there. The GPU test
guards the stale-tag bug of profiles/r05n_e_probe.txt: without the clearing at the
start of a run, a left-over cell whose 2-bit tag equals the expected one passes for a
swept one."""
import pytest

import _seq_tags as st

SIZES = (8300, 8320, 8384, 8256, 8488)  # test_chunked_warm_runs' max_batch values


def calls_of(max_batch):
    n = 3 * max_batch + 77
    return [n // 2, n - n // 2]


def test_batches_of_a_run():
    assert st.run_batches(4096 + 300) == [64] * 64 + [128, 128, 44]
    assert st.run_batches(100) == [64, 36]
    assert st.chunks(3 * 8300 + 77, 8300) == [8300, 8300, 8300, 77]
    assert [st.chunks(n, 8300) for n in calls_of(8300)] == [[8300, 4188], [8300, 4189]]


@pytest.mark.parametrize("max_batch", SIZES)
def test_cleared_runs_never_meet_their_tag(max_batch):
    tr = st.trace(calls_of(max_batch), max_batch, clear=True)
    # four runs, each past the warm-up: batch 1 and batch 64 of every run, batch 65 of the whole chunks
    assert sorted({r[0] for r in tr}) == [0, 1, 2, 3] and {r[1] for r in tr} == {1, 64, 65}
    for run, b, expected, left in tr:
        assert expected in (1, 2, 3) and set(left) == {0}
    assert st.collisions(calls_of(max_batch), max_batch, clear=True) == []


def first_full(max_batch):
    """Per run after the first: (the tag its first full-size batch expects, the tags left in
    the slots past 64 it covers), without the clearing."""
    return [(e, set(left)) for run, b, e, left in st.trace(calls_of(max_batch), max_batch, clear=False)
            if b == 64 and run > 0]


def test_first_full_size_batch_by_hand():
    # 8300: run 0 ends with batch 96 (108 pods, tag 1 + 96 % 3 = 1) over batch 94 (tag 2);
    # run 1's batch 64 (92 pods) waits for 1 + (96 + 64) % 3 = 2 and finds 1 in slots 64..91
    assert first_full(8300)[0] == (2, {1})
    # 8256: run 0 ends with batch 96 of 64 pods, so slots 64..127 of set 0 keep batch 94's
    # tag 2, the tag run 1's batch 64 (70 pods) waits for
    assert first_full(8256)[0] == (2, {2})
    # 8488: run 0 has 99 batches, the last (98, 40 pods, tag 3) leaves batch 96's tag 1 in
    # slots 64..127; run 1's batch 64 (90 pods) waits for 1 + (98 + 64) % 3 = 1
    assert first_full(8488)[0] == (1, {1})


@pytest.mark.parametrize("max_batch,want", [
    # (run, batch) that would take a left-over cell for a swept one without the clearing
    (8300, []), (8320, []),  # sized for the earlier 8,192-pod warm-up: no collision today
    (8384, [(2, 1), (2, 65)]),
    (8256, [(1, 64), (3, 64)]),
    (8488, [(1, 64), (2, 1), (3, 64)]),
])
def test_collisions_without_the_clearing(max_batch, want):
    assert [(r, b) for r, b, e, left in st.collisions(calls_of(max_batch), max_batch, clear=False)] == want
