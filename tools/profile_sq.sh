#!/bin/bash
# SQ issue/occupancy counters of the two render kernels (two --pmc passes, 8 SQ slots each); summarised by
# tools/summarize_sq.py into profiles/<tag>_sq.json.   bash tools/profile_sq.sh r01d   (on an MI355X; output in $PROFILE_OUT, default profile_out/)
set -u
REPO=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r01}
cd /tmp && export TMPDIR=/tmp
cd "$REPO"
export PROFILE_OUT=${PROFILE_OUT:-profile_out}
OUT=$PROFILE_OUT
mkdir -p $OUT
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY --output-format csv -d $OUT/sq1_$TAG -- python3 bench.py --full --no-cpu-baseline --no-seam --no-make-image --no-extras --no-configs --steps 10 --warmup 2 --repeats 1 > $OUT/sq1_$TAG.log 2>&1
rocprofv3 --pmc SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_SCA SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_RD GRBM_GUI_ACTIVE SQ_WAVE_CYCLES --output-format csv -d $OUT/sq2_$TAG -- python3 bench.py --full --no-cpu-baseline --no-seam --no-make-image --no-extras --no-configs --steps 10 --warmup 2 --repeats 1 > $OUT/sq2_$TAG.log 2>&1
rocprofv3 --pmc SQ_INSTS_BRANCH SQ_INSTS_SENDMSG SQ_INSTS_VMEM SQ_INSTS_VALU_TRANS_F32 SQ_INST_CYCLES_SALU SQ_INST_LEVEL_SMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d $OUT/sq3_$TAG -- python3 bench.py --full --no-cpu-baseline --no-seam --no-make-image --no-extras --no-configs --steps 10 --warmup 2 --repeats 1 > $OUT/sq3_$TAG.log 2>&1
rocprofv3 --pmc SQC_DCACHE_REQ SQC_DCACHE_HITS SQC_DCACHE_MISSES SQC_DCACHE_MISSES_DUPLICATE SQC_TC_DATA_READ_REQ SQC_DCACHE_BUSY_CYCLES SQC_TC_STALL SQC_DCACHE_INPUT_VALID_READYB --output-format csv -d $OUT/sq4_$TAG -- python3 bench.py --full --no-cpu-baseline --no-seam --no-make-image --no-extras --no-configs --steps 10 --warmup 2 --repeats 1 > $OUT/sq4_$TAG.log 2>&1
ls $OUT/sq1_$TAG/*/ $OUT/sq2_$TAG/*/ | head
