#!/bin/bash
# where the upload stage's time goes (TS_TIMING=1 TS_STAGE_TIMING=1); usage: bash profiles/stage_timing.sh <tag>
set -e
TAG=${1:-a}
make -s -C teloscope_amd/csrc && make -s -C oracle
mkdir -p gpurun_out
OUT_DIR=${OUT_DIR:-bench_outputs}
mkdir -p "$OUT_DIR"
O=stage_timing_${TAG}
TS_TIMING=1 TS_STAGE_TIMING=1 timeout -k 10 300 python3 bench.py --full --steps 5 --warmup 2 --no-reads --no-cpu-baseline > "$OUT_DIR/$O.json" 2> "$OUT_DIR/$O.txt"
grep -E "upload_pieces|ts_scan_segments" "$OUT_DIR/$O.txt" | head -40
