#!/bin/bash
# HBM traffic of the hot kernels from PMC counters (run on the GPU box):
#   two separate rocprofv3 passes (FETCH_SIZE needs 3 of the 4 TCC slots, WRITE_SIZE 2), counters only
#   with --kernel-trace, as MI355X_MICROARCH.md prescribes.
#   usage: tools/pmc_traffic.sh [tag] [bench.py --full args...]   e.g.  tools/pmc_traffic.sh config5_batch4_env --config 5
#   Output: $OUT_DIR/pmc_<tag>/*.csv, summary.txt, and $OUT_DIR/traffic.json (merge of profiles/traffic.json + this tag)
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT_DIR=${SGR_OUT_DIR:-$ROOT/bench_out}
export TMPDIR=/tmp
TAG=${1:-config2_batch16_env}; shift || true
OUT=$OUT_DIR/pmc_$TAG
mkdir -p $OUT
[ -f $OUT_DIR/traffic.json ] || cp $ROOT/profiles/traffic.json $OUT_DIR/traffic.json
cd /tmp
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 600 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/$c -- python $ROOT/bench.py --full --steps 3 --warmup 1 --reps 1 --no-cpu-baseline --layer-only "$@" > $OUT/$c.log 2>&1
done
cd $ROOT
python tools/parse_pmc.py $OUT $TAG $OUT_DIR/traffic.json > $OUT/summary.txt 2>&1; cat $OUT/summary.txt
find $OUT -name "*.csv" -size +2M -delete
