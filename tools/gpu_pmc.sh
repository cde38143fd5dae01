#!/bin/bash
# PMC passes (HBM traffic) for the headline kernels: separate --pmc runs, kernel-trace only; output under $OUT.
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/build/pmc}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 500 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/$c -o pmc -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/$c.log 2>&1; echo "$c rc=$?"
done
find $OUT -name "*.csv" | head; for f in $(find $OUT -name "*counter_collection*.csv"); do echo $f; head -3 $f; done
