#!/bin/bash
# Variant builds of libminisched_gpu.so with extra -D flags on the sequential engine
# (ms_seq.hip) and its host side (ms_seq_host.cpp), for MINISCHED_LIB=... runs
# (tools/gpu_*.sh). The other objects come from a prior `make`.
# Usage: tools/build_variants.sh NAME "-DFOO=1 ..." [vst|tl]
# -> mini-kube-scheduler_amd/minisched_amd/libminisched_gpu_NAME.so (vst: with the MS_VSTAMPS stamps;
# tl: the per-workgroup step timeline only, e.g. tools/build_variants.sh tl "" tl)
set -e
cd "$(dirname "$0")/../mini-kube-scheduler_amd"
NAME=$1; DEFS=$2; VST=$3
H="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -I../include -Icsrc"
mkdir -p build
if [ "$VST" = vst ]; then
  DEFS="-DMS_VSTAMPS $DEFS"
elif [ "$VST" = tl ]; then  # step timeline only (MS_TIMELINE=<file>; the host side reads it since round 6)
  DEFS="-DMS_TIMELINE_ONLY $DEFS"
fi
$H $DEFS -c csrc/ms_seq.hip -o build/ms_seq_$NAME.o
SEQ_HOST=build/ms_seq_host.o
if [ -n "$DEFS" ]; then  # (the host side reads the stamps: the same -D flags)
  $H $DEFS -c csrc/ms_seq_host.cpp -o build/ms_seq_host_$NAME.o
  SEQ_HOST=build/ms_seq_host_$NAME.o
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o minisched_amd/libminisched_gpu_$NAME.so build/ms_kernels.o build/ms_seq_$NAME.o build/ms_sweep_pp.o build/ms_taint.o build/ms_affinity.o build/ms_capi.o build/ms_cycle.o build/ms_hostarray.o build/ms_nam_tab.o $SEQ_HOST build/ms_comm.o -L/opt/rocm/lib -lrccl
echo built minisched_amd/libminisched_gpu_$NAME.so
