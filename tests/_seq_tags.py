"""The host-side tag sequence of the sequential engine's tile lists, restated
(ms_seq_host.cpp run_sequential: batch_at, merge_tag; ms_seq.hip launch_seq_step:
list_tag, seq_step_merges).

A call is cut into chunks of max_batch pods, each chunk is one run. A run takes
its first 4,096 pods in batches of 64 and the rest in batches of 128. Batch 0 is
swept untagged by a launch; batch b >= 1 is swept by step b - 1 into list set
b & 1, pod slots 0 .. n_b - 1, every cell stamped with the step's 2-bit tag
1 + T % 3, where T is the context's merge_tag: one more for every step that
sweeps a next batch, never reset. The in-step merge of that step takes a cell as
swept once it carries this tag. A run clears both sets first; without that
(clear=False) a cell keeps what an earlier run left, and a warm-up batch
rewrites slots 0..63 only: batch 1 of a run (set 1), its first full-size batch
(batch 64, set 0) and the next one (batch 65, set 1) meet cells of an earlier
run, and take them for swept ones where the tags are equal.
Test infrastructure, never product code.
"""
WARM_PODS, WARM_BATCH, FULL_BATCH = 4096, 64, 128


def chunks(n_pods, max_batch):
    return [min(max_batch, n_pods - a) for a in range(0, n_pods, max_batch)]


def run_batches(n_pods):
    out, s0 = [], 0
    while s0 < n_pods:
        nb = min(WARM_BATCH if s0 < WARM_PODS else FULL_BATCH, n_pods - s0)
        out.append(nb)
        s0 += nb
    return out


def trace(calls, max_batch, clear):
    """calls: pods per ms_schedule_batch call on one context. One record per batch
    whose sweep meets pod slots that its run has not written yet:
    (run, batch, expected, left): the tag the batch waits for and the tags those
    slots hold (0: cleared or untagged). In a run past the warm-up these are batch 1
    (set 1, slots 0..63), batch 64, the first full-size one (set 0, slots 64..),
    and batch 65 (set 1, slots 64..)."""
    cell = [[0] * FULL_BATCH, [0] * FULL_BATCH]  # the tag every (set, pod slot) holds
    merge_tag, out, run = 0, [], 0
    for n_call in calls:
        for n_run in chunks(n_call, max_batch):
            if clear:
                cell = [[0] * FULL_BATCH, [0] * FULL_BATCH]
            fresh = [[False] * FULL_BATCH, [False] * FULL_BATCH]
            nb = run_batches(n_run)
            cell[0][:nb[0]] = [0] * nb[0]  # batch 0: the untagged launch
            fresh[0][:nb[0]] = [True] * nb[0]
            for b in range(1, len(nb)):
                merge_tag += 1
                tag = 1 + merge_tag % 3
                s = b & 1
                left = tuple(cell[s][i] for i in range(nb[b]) if not fresh[s][i])
                if left:
                    out.append((run, b, tag, left))
                cell[s][:nb[b]] = [tag] * nb[b]
                fresh[s][:nb[b]] = [True] * nb[b]
            run += 1
    return out


def collisions(calls, max_batch, clear):
    """The batches that find the tag they wait for in a slot not yet swept in their run."""
    return [r for r in trace(calls, max_batch, clear) if r[2] in r[3]]
