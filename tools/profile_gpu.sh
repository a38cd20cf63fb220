#!/bin/bash
# Runs on a machine with an MI355X: kernel trace + the two HBM PMC passes for bench.py --full, into $PROFILE_OUT (default profile_out/).
#   bash tools/profile_gpu.sh r01        then:  python tools/summarize_profile.py profile_out r01
# Counters are collected in their own runs (no --sys-trace etc. together with --pmc), program directly after `--`.
set -u
REPO=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r01}
cd /tmp && export TMPDIR=/tmp
cd "$REPO"
export PROFILE_OUT=${PROFILE_OUT:-profile_out}
OUT=$PROFILE_OUT
mkdir -p $OUT
python3 bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 bench.py --full --no-cpu-baseline --no-seam --no-make-image --no-extras --no-configs > $OUT/prof_$TAG.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_$TAG -- python3 bench.py --full --no-cpu-baseline --no-seam --no-make-image --no-extras --no-configs --steps 10 --warmup 2 --repeats 1 > $OUT/pmc_fetch_$TAG.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_$TAG -- python3 bench.py --full --no-cpu-baseline --no-seam --no-make-image --no-extras --no-configs --steps 10 --warmup 2 --repeats 1 > $OUT/pmc_write_$TAG.log 2>&1
tail -c 2500 $OUT/bench_$TAG.json
