#!/bin/bash
# K3 on a side stream beside the next step's K1 (TCBEE_BENCH_ASYNC=1) vs in line, config 3,
# alternating processes (round 6, profiles/r06_async_ids_ab.log). Output under $OUT.
set -u
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for i in 1 2; do
  for a in 0 1; do
    TCBEE_BENCH_ASYNC=$a timeout -k 10 200 python bench.py --full --no-extra --no-cpu > "$OUT/async_${a}_$i.json" 2> "$OUT/async_${a}_$i.err" || exit 1
    python3 -c "import json,sys;d=json.loads(open('$OUT/async_${a}_$i.json').read().strip().splitlines()[-1]);print('async=$a run $i',d['value'],d['ms_per_step'],d['roofline']['k1_ms'],d['check']['full_bit_exact'])"
  done
done
