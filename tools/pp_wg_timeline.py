#!/usr/bin/env python3
"""Wave timeline of K1 pp (k_sweep_nunn_pp) at config C from the `make pp-timeline` build.

The diagnostic library (minisched_amd/libminisched_gpu_pptl.so, ms_sweep_pp.hip under
-DMS_PP_TIMELINE) appends one record per launch to the file named by MS_PP_TIMELINE: 8 u32
of header (magic "PPTL", version, workgroups, waves, stamps per wave, chunk, pods, wave
slots per workgroup), then workgroups x 16 x stamps u64: s_memtime at the stamp points
(the kTl* enum there, mirrored below), one pair of s_memrealtime (100 MHz), and the wave's
candidate hashes per lane. A stamp of 0 was never taken (a wave without tiles of a digit,
an unsorted chunk's sort barriers, planes that were not loaded).

Run: MINISCHED_LIB=.../libminisched_gpu_pptl.so python tools/pp_wg_timeline.py [--out f.json]
     [--key after]  -- config C once warm, steps 5-14 recorded, medians over workgroups and
waves printed and merged into the JSON under the key. parse() / phases() are the parser
(tests/test_pp_timeline_parse.py).
"""
import argparse
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAGIC = 0x4C545050
ENTRY, BAR1, BAR2, BAR3, PLANES, BAR4, SWEEP_END, SWEEP_BAR, FINAL, END, REAL0, REAL1 = range(12)
DIGIT0, HASHES = 12, 42
N_SLOTS = 10
VALU_PER_HASH = 5.5  # sweep_list_pods' full block per pod and entry pair: 2 add, 4 xor-shift, 4 mul, 1 max3
REALTIME_HZ = 100e6


def parse(buf):
    """The records of a timeline file: dicts with the header fields and `t`, a
    (workgroups, waves, stamps) uint64 array (the unused wave slots dropped)."""
    out, off = [], 0
    while off < len(buf):
        if len(buf) - off < 32:
            raise ValueError("truncated header")
        magic, ver, n_wg, waves, stamps, chunk, n_pods, slots = struct.unpack_from("<8I", buf, off)
        if magic != MAGIC or ver != 1:
            raise ValueError(f"bad record header at byte {off}")
        if not 0 < waves <= slots or stamps <= HASHES:
            raise ValueError("bad geometry")
        off += 32
        n = n_wg * slots * stamps
        if len(buf) - off < 8 * n:
            raise ValueError("truncated record")
        t = np.frombuffer(buf, dtype="<u8", count=n, offset=off).reshape(n_wg, slots, stamps)[:, :waves, :]
        off += 8 * n
        out.append({"workgroups": n_wg, "waves": waves, "stamps": stamps, "chunk": chunk, "pods": n_pods, "t": t})
    return out


def _span(t, a, b):
    # t[..., b] - t[..., a] in ticks where both stamps were taken, else NaN
    x, y = t[..., a].astype(np.float64), t[..., b].astype(np.float64)
    return np.where((x > 0) & (y > 0), y - x, np.nan)


def phases(rec, ghz):
    """Phase figures of one record, medians over workgroups and waves, in microseconds
    (ghz: the shader clock, for the issue efficiency). Waves that took no stamp (their
    workgroup had no pod) are left out."""
    t = rec["t"]
    live = t[..., END] > 0
    # s_memtime ticks per second, from the wave's own pair of s_memrealtime
    real = _span(t, REAL0, REAL1)
    mem = _span(t, ENTRY, END)
    ok = live & (real > 0)
    hz = float(np.nanmedian((mem / real)[ok])) * REALTIME_HZ
    us = 1e6 / hz

    def med(x, sel=live):
        v = x[sel]
        v = v[~np.isnan(v)]
        return float(np.median(v)) * us if len(v) else None

    issued = t[..., DIGIT0:DIGIT0 + 3 * N_SLOTS:3].astype(np.float64)
    landed = t[..., DIGIT0 + 1:DIGIT0 + 3 * N_SLOTS:3].astype(np.float64)
    switch = np.where((issued > 0) & (landed > 0), landed - issued, 0.0).sum(axis=-1)
    sweep = _span(t, BAR4, SWEEP_END)
    hashing = sweep - switch
    out = {
        "memtime_mhz": hz / 1e6,
        "waves_recorded": int(live.sum()),
        "prologue_us": med(_span(t, ENTRY, BAR4)),
        "to_barrier1_us": med(_span(t, ENTRY, BAR1)),
        "barrier1_to_2_us": med(_span(t, BAR1, BAR2)),
        "barrier2_to_3_us": med(_span(t, BAR2, BAR3)),
        "barrier3_to_4_us": med(_span(t, BAR3, BAR4)),
        "planes_landed_after_barrier3_us": med(_span(t, BAR3, PLANES)),
        "switch_wait_sum_us": med(switch),
        "hashing_us": med(hashing),
        "sweep_barrier_wait_us": med(_span(t, SWEEP_END, SWEEP_BAR)),
        "final_and_epilogue_us": med(_span(t, SWEEP_BAR, END)),
        "kernel_wave_us": med(mem),
    }
    wave = np.arange(t.shape[1])
    out["sweep_barrier_wait_by_simd_us"] = [med(_span(t, SWEEP_END, SWEEP_BAR)[:, wave % 4 == k], live[:, wave % 4 == k])
                                            for k in range(min(4, t.shape[1]))]
    # issue efficiency of the hashing phase, per SIMD of a workgroup (waves w, w + 4, ..):
    # the waves' hash instructions x 4 cycles over the cycles from the sweep's first
    # barrier to the SIMD's last wave done, less its longest switch wait
    instr = t[..., HASHES].astype(np.float64) * VALU_PER_HASH
    eff = []
    for k in range(min(4, t.shape[1])):
        m = wave % 4 == k
        h = np.where(live[:, m], sweep[:, m] - switch[:, m], np.nan)
        span = np.nan_to_num(h, nan=0.0).max(axis=1)  # (0: a workgroup without pods)
        work = np.where(live[:, m], instr[:, m], 0.0).sum(axis=1) * 4.0
        cyc = span * us * 1e-6 * ghz * 1e9
        good = cyc > 0
        eff.append(float(np.median(work[good] / cyc[good])) if good.any() else None)
    out["hash_issue_efficiency_by_simd"] = eff
    return out


def summarise(recs, ghz):
    """Medians over the records of every figure of phases()."""
    per = [phases(r, ghz) for r in recs]
    out = {}
    for k in per[0]:
        vals = [p[k] for p in per]
        if isinstance(vals[0], list):
            out[k] = [None if any(v[i] is None for v in vals) else float(np.median([v[i] for v in vals]))
                      for i in range(len(vals[0]))]
        else:
            out[k] = None if any(v is None for v in vals) else float(np.median(vals))
    out["records"] = len(per)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file to merge the figures into")
    ap.add_argument("--key", default="after", help="key in that file (before / after)")
    ap.add_argument("--raw", default="/tmp/pp_timeline.bin", help="where the library writes the records")
    ap.add_argument("--ghz", type=float, default=None, help="shader clock (default: profiles/r16a_pmc_C.json)")
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--pods", type=int, default=100_000)
    args = ap.parse_args()
    ghz = args.ghz
    if ghz is None:
        ghz = json.load(open(os.path.join(ROOT, "profiles", "r16a_pmc_C.json")))["effective_clock_ghz"]
    sys.path.insert(0, os.path.join(ROOT, "mini-kube-scheduler_amd"))
    import torch

    from minisched_amd import _lib, synth

    if "pptl" not in os.path.basename(_lib.LIB_PATH):
        sys.exit("set MINISCHED_LIB to the `make pp-timeline` library")
    if os.path.exists(args.raw):
        os.remove(args.raw)
    os.environ.pop("MS_PP_TIMELINE", None)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    with _lib.Engine(max_nodes=args.nodes, seed=1) as eng:
        eng.upsert(np.arange(args.nodes), synth.nodes(args.nodes, seed=1))
        eng.flush()
        pods = torch.from_numpy(synth.pods(args.pods, seed=1).view(np.uint8).copy()).to(dev)
        res = torch.empty(args.pods * 24, dtype=torch.uint8, device=dev)
        for step in range(15):  # steps 5-14 recorded (the library reads the variable at every launch)
            if step == 5:
                os.environ["MS_PP_TIMELINE"] = args.raw
            eng.select_batch_device(args.pods, pods.data_ptr(), res.data_ptr(), s.cuda_stream)
            s.synchronize()
        os.environ.pop("MS_PP_TIMELINE", None)
    recs = parse(open(args.raw, "rb").read())
    os.remove(args.raw)
    fig = summarise(recs, ghz)
    fig["shader_ghz"] = ghz
    fig["workgroups"], fig["waves"], fig["chunk"] = recs[0]["workgroups"], recs[0]["waves"], recs[0]["chunk"]
    print(json.dumps(fig, indent=1))
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc[args.key] = fig
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
