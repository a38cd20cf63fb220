#!/bin/bash
# Everything profiles/<tag>_* is made of, in one run on a machine with an MI355X:  bash tools/profile_all.sh r04j   (output in $PROFILE_OUT, default profile_out/)
# then: python3 tools/summarize_profile.py profile_out <tag>; python3 tools/summarize_sq.py profile_out <tag>; copy the bench / log files into
# profiles/; run bench.py once more ON the stamped tree and keep its line as profiles/<tag>_bench.json (its `from_profiles` then matches).
set -u
REPO=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r04d}
cd "$REPO"
export PROFILE_OUT=${PROFILE_OUT:-profile_out}
OUT=$PROFILE_OUT
mkdir -p $OUT
bash tools/profile_gpu.sh $TAG > $OUT/pg_$TAG.log 2>&1; echo "profile_gpu done"
bash tools/profile_sq.sh $TAG > $OUT/ps_$TAG.log 2>&1; echo "profile_sq done"
for wl in config2 make_image config5 config5_100k; do
  python3 bench.py --full --workload $wl --no-cpu-baseline --no-seam --no-make-image --no-extras --no-configs > $OUT/bench_${TAG}_$wl.json 2> $OUT/bench_${TAG}_$wl.err; echo "bench $wl done"
done
python3 tools/f64_time.py > $OUT/f64_time_$TAG.log 2>&1; echo "f64 done"
python3 tools/wave_timeline.py 800 600 1 8 > $OUT/wave_timeline_800x600_$TAG.log 2>&1
WAVE_TIMELINE_JSON=$OUT/roofline_waves.json WAVE_TIMELINE_TAG=$TAG python3 tools/wave_timeline.py 1920 1080 1 8 > $OUT/wave_timeline_1080p_$TAG.log 2>&1; echo "timelines done"
python3 tools/shard_expect.py > $OUT/shard_render_times_$TAG.log 2>&1; echo "shard done"
tail -3 $OUT/shard_render_times_$TAG.log
