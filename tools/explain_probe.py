#!/usr/bin/env python3
"""Times ms_explain_device at the benchmark shapes: 16 pods over the whole table
for plugin sets 0 (100,000 rows), 3 and 4 (50,000 rows), with rows and summary
only. Call time from device events around the call on a caller stream, after a
warm-up of the same shape; per shape the median, minimum and 10th / 90th
percentile of the repeats, and the store floor of the rows written
(n_pods x n_nodes x 24 bytes over the plain-store rate of HBM, 6.0 TB/s).

    python tools/explain_probe.py [--pods 16] [--repeats 200] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mini-kube-scheduler_amd"))

from minisched_amd import _lib, synth  # noqa: E402

HBM_STORE_BYTES_PER_S = 6.0e12
SHAPES = ((_lib.PLUGINS_NU_NN, 100_000), (_lib.PLUGINS_NU_TT_NN, 50_000), (_lib.PLUGINS_NU_NN_NAM, 50_000))
N_SETS = 64


def time_calls(call, stream, warmup, repeats):
    import torch

    for _ in range(warmup):
        call()
    stream.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    with torch.cuda.stream(stream):
        for a, b in ev:
            a.record()
            call()
            b.record()
    stream.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return dict(median_us=float(np.median(us)), min_us=float(us.min()), p10_us=float(np.percentile(us, 10)),
                p90_us=float(np.percentile(us, 90)), repeats=repeats)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    out = []
    for ps, n in SHAPES:
        nr = synth.nodes(n, seed=1, taints=ps == _lib.PLUGINS_NU_TT_NN, labels=ps == _lib.PLUGINS_NU_NN_NAM)
        pr = synth.pods(a.pods, seed=1, taints=ps == _lib.PLUGINS_NU_TT_NN,
                        term_sets=N_SETS if ps == _lib.PLUGINS_NU_NN_NAM else 0)
        pods_d = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
        rows_d = torch.empty(a.pods * n * _lib.EXPLAIN_ROW.itemsize, dtype=torch.uint8, device=dev)
        sums_d = torch.empty(a.pods * _lib.EXPLAIN_SUMMARY.itemsize, dtype=torch.uint8, device=dev)
        with _lib.Engine(max_nodes=n, plugin_set=ps, seed=1) as e:
            e.upsert(np.arange(n), nr)
            if ps == _lib.PLUGINS_NU_NN_NAM:
                e.nam_term_sets_ext(synth.nam_term_sets_ext(N_SETS, seed=1))
                e.nam_required_sets(synth.nam_required_sets(N_SETS, seed=1))
            e.flush()
            row_bytes = a.pods * n * _lib.EXPLAIN_ROW.itemsize
            floor_us = row_bytes / HBM_STORE_BYTES_PER_S * 1e6
            for what, rows, sums in (("rows+summaries", rows_d.data_ptr(), sums_d.data_ptr()),
                                     ("rows", rows_d.data_ptr(), 0), ("summaries", 0, sums_d.data_ptr())):
                t = time_calls(lambda: e.explain_device(a.pods, pods_d.data_ptr(), 0, n if rows else 0, rows, sums,
                                                        s.cuda_stream), s, a.warmup, a.repeats)
                t.update(plugin_set=ps, rows=n, pods=a.pods, call=what)
                if rows:
                    t.update(row_bytes=row_bytes, store_floor_us=floor_us, floor_fraction=floor_us / t["median_us"])
                out.append(t)
                print(json.dumps(t), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
