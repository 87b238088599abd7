#!/usr/bin/env python3
"""One rank's step of the multi-term NodeAffinity set (MS_PLUGINS_NU_NN_NAM) over
node shards, on one GPU, two ways, alternated run by run in one process:

  resumed    the in-library cycle (ms_sharded_submit on a joined context): class
             records, one all-gather, the keys pass RESUMING from the first
             pass's scratch, keys and filter bytes reduce-scattered, slice decode
             (the variant that ran the class pass again is recorded as
             profiles/r15a_nam_class_pass_again.patch, with its figures in
             profiles/r15a_nam_inlibrary.txt);
  pod_form   the caller-collective form on an unjoined context of the same
             shard: ms_nam_segment_device + ms_nam_keys_device (one record per
             pod; the caller's own all-gather and MAX are NOT included).

The in-library forms run through the test-only loopback build in its solo mode
(MS_LB_SOLO=1, as tools/step_probe_rank.py): ONE context joins a G-rank
communicator as rank G-1 with that rank's shard, so the collectives move one
rank's bytes on the device and say nothing about xGMI. Shape: 50k nodes x 100k
pods, 64 general term sets (bench.py's NAM_ext inputs), G = 4 by default.
Prints one JSON object per run and a summary (median, min..max spread per form).
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mini-kube-scheduler_amd"))
os.environ["MS_LB_SOLO"] = "1"


def main():
    import torch

    from minisched_amd import _lib, sharded, synth

    N, P, SETS, seed = 50_000, 100_000, 64, 1
    G = int(os.environ.get("PROBE_G", 4))
    K = int(os.environ.get("PROBE_STEPS", 20))
    RUNS = int(os.environ.get("PROBE_RUNS", 6))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    r = G - 1
    lo, hi = sharded.shard_bounds(N, r, G)
    nr = synth.nodes(hi - lo, seed=seed, start=lo, labels=True)
    pr = synth.pods(P, seed=seed, term_sets=SETS)
    tse = synth.nam_term_sets_ext(SETS, seed=seed)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    sid = pr["pref_zone"].astype(np.int64) | pr["pref_weight"].astype(np.int64) << 8
    classes = len(set(zip(sid.tolist(), pr["tolerates_unschedulable"].tolist())))
    C = min(P, 2 * (SETS + 1))
    print(json.dumps(dict(shape=f"{N} nodes x {P} pods, {SETS} term sets, rank {r} of {G}: rows {hi - lo}",
                          classes=classes, class_records_per_rank=C, allgather_bytes_class_form=C * _lib.NAM_SEG_BYTES,
                          allgather_bytes_pod_form=P * _lib.NAM_SEG_BYTES)))

    def engine(lib):
        e = _lib.Engine(max_nodes=hi - lo, plugin_set=_lib.PLUGINS_NU_NN_NAM, node_base=lo, seed=seed, lib=lib)
        e.nam_term_sets_ext(tse)
        e.upsert(np.arange(lo, hi), nr)
        e.flush()
        return e

    def timed(step, finish):
        for _ in range(3):
            step()
        finish()
        s.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(K):
            step()
        finish()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) / K

    lb = _lib.load(_lib.LOOPBACK_LIB_PATH)
    joined = engine(lb)
    joined.comm_init(_lib.comm_id_create(lb), r, G)
    cyc = sharded.ShardedCycle(joined, N, P, pods, s)
    assert cyc.library
    forms = {"resumed": (cyc.step, cyc.finish)}
    keep = [joined]
    e = engine(lb)  # unjoined: the caller-collective form
    segs = torch.zeros(G * P * _lib.NAM_SEG_BYTES, dtype=torch.uint8, device=dev)
    keys = torch.zeros(P, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for g in range(G):  # (every shard's block holds valid records: this shard's own, as in the solo collectives)
        e.nam_segment_device(P, pods.data_ptr(), segs.data_ptr() + g * P * _lib.NAM_SEG_BYTES, s.cuda_stream)
    s.synchronize()

    def pod_step():
        e.nam_segment_device(P, pods.data_ptr(), segs.data_ptr() + r * P * _lib.NAM_SEG_BYTES, s.cuda_stream)
        e.nam_keys_device(P, pods.data_ptr(), G, r, segs.data_ptr(), keys.data_ptr(), s.cuda_stream)

    forms["pod_form"] = (pod_step, lambda: None)
    keep.append(e)
    runs = {k: [] for k in forms}
    for i in range(RUNS):  # alternated: run i of every form before run i + 1 of any
        for name, (step, finish) in forms.items():
            ms = timed(step, finish)
            runs[name].append(ms)
            print(json.dumps(dict(run=i, form=name, ms_per_step=round(ms, 4))))
    for name, v in runs.items():
        print(json.dumps(dict(form=name, runs=len(v), median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4),
                              max_ms=round(max(v), 4), spread_ms=round(max(v) - min(v), 4))))
    for e in keep:
        e.close()


if __name__ == "__main__":
    main()
