#!/bin/bash
# PMC of config E's speculative sweep inside the fused step (k_seq_step), and the kernels' times.
# Counters and the kernel trace are collected in runs of their own.
set -o pipefail
export TMPDIR=/tmp
OUT=gpurun_out/pmc_e; rm -rf $OUT; mkdir -p $OUT
B="python tools/bench_configs.py --configs E --reps 1 --e-pods 20000"
C="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE"
timeout -s KILL 240 rocprofv3 --pmc $C -d $OUT/sqf -o run --output-format csv -- $B > /dev/null 2> $OUT/sqf.err || { echo sqf pass failed; tail $OUT/sqf.err; exit 1; }
timeout -s KILL 240 rocprofv3 --kernel-trace --stats -d $OUT/stf -o run --output-format csv -- $B > /dev/null 2> $OUT/stf.err || { echo stats failed; tail $OUT/stf.err; exit 1; }
OUT=$OUT python3 - <<'PY'
import csv, glob, collections, os, re
out = os.environ['OUT']
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(out + '/sqf/**/*counter_collection.csv', recursive=True):
    for r in csv.DictReader(open(f)):
        m = re.search(r'(k_\w+)', r['Kernel_Name']); k = m.group(1) if m else r['Kernel_Name'][:30]
        agg[k][r['Counter_Name']].append(float(r['Counter_Value']))
for k, d in agg.items():
    if any(x in k for x in ('topk', 'validate', 'merge', 'seq_step')):
        print('sqf', k, {c: round(sum(v)/len(v)) for c, v in d.items()})
for f in glob.glob(out + '/stf/**/*kernel_stats.csv', recursive=True):
    for r in csv.DictReader(open(f)):
        print('stf', 'stats', r['Name'][:50], r['Calls'], r['AverageNs'])
PY
