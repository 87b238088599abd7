#!/usr/bin/env python3
"""NodeAffinity as a filter (ms_nam_required_sets) at bench.py --full's NAM shape,
50k nodes x 100k pods, 64 sets, batched, ms_select_batch_device.

Times three workloads the way bench.py's `configs` do (one warm-up, then the
median wall time of 5 synchronised cycles):
  NAM      synth.nam_term_sets      (bench.py configs.NAM)
  NAM_ext  synth.nam_term_sets_ext  (bench.py configs.NAM_ext)
  NAM_req  NAM_ext plus synth.nam_required_sets (this library only), checked on
           a pod prefix against the tombstone reference of tests/_nam_required_ref.py
--ab OTHER.so: an A/B of the two row kernels that changed. OTHER is a build of
the library without the feature; both are loaded into this one process and run
alternately, --rounds times each, on the same device buffers, and the two
libraries' NAM / NAM_ext results must be byte-identical.
--resources: VGPRs and scratch of k_nam_seg / k_nam_fscore / k_nam_flags from
the compiler's resource remarks (compiles ms_affinity.hip; no GPU needed).
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mini-kube-scheduler_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def resources():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(PKG, "csrc"), "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(PKG, "csrc", "ms_affinity.hip"), "-o", os.devnull],
                         capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: \S*?(k_nam_[a-z]+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    return {k: v for k, v in res.items() if k in ("k_nam_seg", "k_nam_fscore", "k_nam_flags")}


def load_other(path, _lib):
    """A build that may lack the newest symbols: bind the ones it has."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def median_time(fn, sync, reps=5):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", default=None, metavar="OTHER.so")
    ap.add_argument("--only", default=None, choices=["other", "new"],
                    help="with --ab: run that library alone (per-kernel traces of one build)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prefix", type=int, default=2000)
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    if args.resources:
        print(json.dumps({"resources": resources()}))
        return
    import torch

    from minisched_amd import _lib, synth

    N, P, K = args.nodes, args.pods, args.sets
    dev = torch.device("cuda:0")
    nr = synth.nodes(N, seed=args.seed, labels=True)
    pr = synth.pods(P, seed=args.seed, term_sets=K)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    ts16, tse = synth.nam_term_sets(K, seed=args.seed), synth.nam_term_sets_ext(K, seed=args.seed)
    rq = synth.nam_required_sets(K, seed=args.seed)
    libs = {"new": _lib.load()}
    if args.ab:
        libs = {"other": load_other(args.ab, _lib), "new": libs["new"]}
        if args.only:
            libs = {args.only: libs[args.only]}

    def engine(lib, install):
        e = _lib.Engine(max_nodes=N, plugin_set=_lib.PLUGINS_NU_NN_NAM, seed=args.seed, device=0, lib=lib)
        install(e)
        e.upsert(np.arange(N), nr)
        e.flush()
        return e

    work = {"NAM": lambda e: e.nam_term_sets(ts16), "NAM_ext": lambda e: e.nam_term_sets_ext(tse)}
    runs, outs = {}, {}
    engines = {(ln, wn): engine(lib, inst) for ln, lib in libs.items() for wn, inst in work.items()}
    if "new" in libs:
        engines[("new", "NAM_req")] = engine(libs["new"], lambda e: (e.nam_term_sets_ext(tse), e.nam_required_sets(rq)))
    try:
        for _ in range(args.rounds):  # alternately: every library and workload once per round
            for key, e in engines.items():
                res = outs.setdefault(key, torch.empty(P * 24, dtype=torch.uint8, device=dev))
                ms = median_time(lambda: e.select_batch_device(P, pods.data_ptr(), res.data_ptr()), torch.cuda.synchronize)
                runs.setdefault(key, []).append(ms)
    finally:
        for e in engines.values():
            e.close()
    out = {"nodes": N, "pods": P, "sets": K, "rounds": args.rounds, "reps_per_round": 5}
    for (ln, wn), ms in runs.items():
        out[f"{wn}/{ln}"] = {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "rounds_ms": ms}
    if len(libs) == 2:
        out["identical"] = {wn: bool(torch.equal(outs[("other", wn)], outs[("new", wn)])) for wn in work}
    if "new" not in libs:
        print(json.dumps(out))
        return
    import _nam_required_ref as ref
    import _oracle

    n = min(args.prefix, P)
    got = outs[("new", "NAM_req")].cpu().numpy().view(_lib.RESULT)[:n]
    want = ref.schedule_tombstone(_oracle, nr, pr[:n], tse, rq, seed=args.seed, literal=False)
    out["NAM_req_parity_prefix"] = all(
        np.array_equal(np.asarray(got[k]).astype(np.int64), want[kw].astype(np.int64))
        for k, kw in (("node", "node"), ("code", "code"), ("score", "score"), ("plugin_mask", "mask")))
    out["NAM_req_prefix_fit_errors"] = int((want["code"] == 2).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
