#!/bin/bash
# pcie_inclusive legs of bench.py with the packed upload on and off
set -e
make -s -C teloscope_amd/csrc && make -s -C oracle
mkdir -p gpurun_out
OUT=gpurun_out/packed_${1:-a}.txt
ERR=${OUT%.txt}_err.txt
: > $OUT
for p in ${PACKED:-0 1}; do
  echo "TS_PACKED_UPLOAD=$p" >> $OUT
  TS_TIMING=1 TS_PACKED_UPLOAD=$p python3 bench.py --full --no-cpu-baseline --no-reads --steps 5 --warmup 2 2> "$ERR" | python3 -c "
import json,sys
for l in sys.stdin:
    if l.startswith('{'):
        d=json.loads(l)['pcie_inclusive']
        print('   blocks %.1f  matches %.1f  multi %.1f Gbases/s' % (d['blocks_windows_counts']['gbases_per_s'], d['with_match_vectors']['gbases_per_s'], d['writer_view_multi']['gbases_per_s']))
" >> $OUT
  grep "ts_scan_segments" "$ERR" | tail -4 | cut -c1-330 >> $OUT
done
cat $OUT
