#!/bin/bash
# One counter-only pass (rocprofv3 --pmc, no tracing) of tools/experiments/front_end_split.py per library build, then its table.
# usage: [VBX_OUT_DIR=dir] tools/experiments/front_end_split.sh name=lib.so ...      (output under bench_out/ by default; names: full_parent full_new p1..p6 n2..n6, see front_end_split.py)
# Builds: make -C vox_box.rs_amd BUILD=build_p3 LIB=lib/libvoxbox_hip_p3.so EXTRA="-DVBX_EXP_FRONT_END_ONCE=0 -DVBX_EXP_STOP=3" (n3: without the first flag)
R=$(cd "$(dirname "$0")/../.." && pwd); O=${VBX_OUT_DIR:-$R/bench_out}/front_end_split; rm -rf "$O"; mkdir -p "$O"; cd "$R"
export TMPDIR=${TMPDIR:-/tmp}
for spec in "$@"; do
    name=${spec%%=*}; lib=${spec#*=}
    VBX_LIB_PATH=$(realpath "$lib") timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES SQ_WAVE_CYCLES \
        --output-format csv -d "$O/$name" -- python3 tools/experiments/front_end_split.py run > "$O/$name.log" 2>&1
    rc=$?
    echo "$name: exit $rc"
    if [ $rc -ne 0 ]; then tail -20 "$O/$name.log"; exit $rc; fi
done
python3 tools/experiments/front_end_split.py table "$O" | tee "$O/front_end_split.txt"
