#!/usr/bin/env python3
"""Times ms_explain_device at the benchmark shapes: 16 pods over the whole table
for plugin sets 0 (100,000 rows), 3 and 4 (50,000 rows), with rows and summary
only. Call time from device events around the call on a caller stream, after a
warm-up of the same shape; per shape the median, minimum and 10th / 90th
percentile of the repeats, and the store floor of the rows written
(n_pods x n_nodes x 24 bytes over the plain-store rate of HBM, 6.0 TB/s).

    python tools/explain_probe.py [--pods 16] [--repeats 200] [--out FILE.json]

--sharded G times the collective call instead: G loopback contexts on one GPU
(the test-only library, one host thread per rank), each holding a shard of
12,500 rows, every rank asking for its own rows and the summaries, for plugin
sets 0 and 4; and in the same run ms_explain_device on a context that is not
joined and holds the same 12,500 rows. Both are host wall times of the call
plus the synchronise of its stream, on rank 0 (the loopback's collectives
rendezvous on the host, so device events around one rank's call would not see
the wait for the others). The loopback exchange is a same-GPU copy after a host
barrier of G threads: what xGMI and RCCL cost instead is not measured here.
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


SHARD_ROWS = 12_500


def wall_stats(us, **more):
    us = np.asarray(us)
    return dict(median_us=float(np.median(us)), min_us=float(us.min()), p10_us=float(np.percentile(us, 10)),
                p90_us=float(np.percentile(us, 90)), repeats=len(us), **more)


def sharded(a):
    """The collective call on G loopback ranks against the single-context call on one shard's rows."""
    import threading
    import time

    import torch

    lib = _lib.load(_lib.LOOPBACK_LIB_PATH)
    G, n, dev = a.sharded, SHARD_ROWS, torch.device("cuda:0")
    out = []
    for ps in (_lib.PLUGINS_NU_NN, _lib.PLUGINS_NU_NN_NAM):
        nam = ps == _lib.PLUGINS_NU_NN_NAM
        nr = synth.nodes(G * n, seed=1, labels=nam)
        pr = synth.pods(a.pods, seed=1, term_sets=N_SETS if nam else 0)
        host_pods = pr.view(np.uint8).copy()

        def engine(lo):
            e = _lib.Engine(max_nodes=n, plugin_set=ps, node_base=lo, seed=1, lib=lib)
            e.upsert(np.arange(lo, lo + n), nr[lo:lo + n])
            if nam:
                e.nam_term_sets_ext(synth.nam_term_sets_ext(N_SETS, seed=1))
                e.nam_required_sets(synth.nam_required_sets(N_SETS, seed=1))
            e.flush()
            return e

        def timed(call, s, sync_ranks):
            pods_d = torch.from_numpy(host_pods).to(dev)
            rows_d = torch.empty(a.pods * n * _lib.EXPLAIN_ROW.itemsize, dtype=torch.uint8, device=dev)
            sums_d = torch.empty(a.pods * _lib.EXPLAIN_SUMMARY.itemsize, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            us = []
            for k in range(a.warmup + a.repeats):
                sync_ranks()  # every rank starts the call together
                t0 = time.perf_counter()
                call(pods_d.data_ptr(), rows_d.data_ptr(), sums_d.data_ptr(), s.cuda_stream)
                s.synchronize()
                if k >= a.warmup:
                    us.append((time.perf_counter() - t0) * 1e6)
            return us

        with engine(0) as e:
            s = torch.cuda.Stream(device=dev)
            us = timed(lambda p, r, m, st: e.explain_device(a.pods, p, 0, n, r, m, st), s, lambda: None)
        out.append(wall_stats(us, plugin_set=ps, rows=n, pods=a.pods, call="ms_explain_device, not joined"))
        print(json.dumps(out[-1]), flush=True)

        cid = _lib.comm_id_create(lib)
        gate = threading.Barrier(G)
        got, errs = [None] * G, [None] * G

        def rank(r):
            try:
                with engine(r * n) as e:
                    e.comm_init(cid, r, G)
                    s = torch.cuda.Stream(device=dev)
                    got[r] = timed(lambda p, rw, m, st: e.explain_sharded_device(a.pods, p, r * n, n, rw, m, st), s,
                                   gate.wait)
            except BaseException as x:  # reported below
                errs[r] = repr(x)
                gate.abort()

        ts = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(600)
        if any(errs) or any(t.is_alive() for t in ts):
            raise SystemExit(f"sharded probe failed: {errs}")
        out.append(wall_stats(got[0], plugin_set=ps, rows=n, pods=a.pods, world=G,
                              call="ms_explain_sharded_device, loopback, rank 0"))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sharded", type=int, default=0, metavar="G",
                    help="time the collective call on G loopback ranks of 12,500 rows each")
    a = ap.parse_args()
    if a.sharded:
        out = sharded(a)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
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
