#!/bin/bash
# A/B of the split first-layer projection (per-gene table + positional GEMM) on the C2 bench, same box
for split in True False True False; do
  python -c "
import sys, runpy, torch
from segger_amd import ops
ops.SPLIT_FIRST_LAYER = $split
sys.argv = ['bench.py', '--full', '--no-strong', '--no-f32', '--no-cpu-baseline']
runpy.run_path('bench.py', run_name='__main__')" 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('split $split', round(d['ms_per_step'],3), round(d['predict']['ms_per_batch'],3))"
done
