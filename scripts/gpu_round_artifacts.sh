#!/bin/bash
# Everything the round's measurement artifacts come from, in one GPU call: the full `-m gpu` suite (parity ledger, per-parameter gradient-error tables,
# RCCL world-1 check), the bench workloads (headline with the CPU baseline; config E with bf16 and fp8 attention; UniDisc-S), the rocprofv3 kernel-trace
# summaries of all three workloads and the two PMC passes (HBM traffic, MFMA utilisation) of the headline command, the CU-reservation measurement.
# Usage: bash scripts/gpu_round_artifacts.sh r03     (outputs under $UDM_OUT, default out/, copied to profiles/ by scripts/collect_profiles.sh)
TAG=${1:-r06}; export TAG; R=$(pwd); export UDM_OUT=${UDM_OUT:-$R/out}; mkdir -p $UDM_OUT; export TMPDIR=/tmp
cd $R
[ -n "$SKIP_TESTS" ] || UDM_DUMP_GRAD_ERRS=$UDM_OUT/graderrs_$TAG UDM_LEDGER=$UDM_OUT/parity_ledger_$TAG.json timeout 2400 python -m pytest tests -m gpu -q -p no:cacheprovider --timeout 1500 2>&1 | tail -15 > $UDM_OUT/gputests_$TAG.log
timeout 900 python bench.py --full --steps 25 --warmup 5 > $UDM_OUT/bench_1.4b_b8_$TAG.json 2> $UDM_OUT/bench_1.4b_b8_$TAG.err
# every workload of SURVEY §8(d) with its cpu_baseline in the same run
timeout 900 python bench.py --full --workload unidisc-s-l384 --steps 12 --warmup 3 > $UDM_OUT/bench_unidisc_s_b64_$TAG.json 2>/dev/null
timeout 900 python bench.py --full --workload unidisc-1.4b-interleaved-l4608 --steps 12 --warmup 3 > $UDM_OUT/bench_1.4b_interleaved_l4608_b2_$TAG.json 2>/dev/null
timeout 900 python bench.py --full --workload unidisc-1.4b-interleaved-l4608 --batch 1 --steps 12 --warmup 3 > $UDM_OUT/bench_1.4b_interleaved_l4608_b1_$TAG.json 2>/dev/null
timeout 900 python bench.py --full --workload unidisc-1.4b-l1280-adaln --steps 12 --warmup 3 > $UDM_OUT/bench_1.4b_adaln_b8_$TAG.json 2>/dev/null
timeout 600 python bench.py --full --steps 12 --warmup 3 --no-cpu-baseline --table-steps 0 --hog-cus 16 > $UDM_OUT/bench_1.4b_b8_16cus_held_$TAG.json 2>/dev/null
bash scripts/gpu_prof.sh $TAG > $UDM_OUT/prof_summary_$TAG.log 2>&1
cp $UDM_OUT/kernel_stats_$TAG.csv $UDM_OUT/kernel_stats_1.4b_b8_$TAG.csv
EXTRA="--workload unidisc-1.4b-interleaved-l4608" bash scripts/gpu_prof.sh ${TAG}e > $UDM_OUT/prof_summary_${TAG}e.log 2>&1
EXTRA="--workload unidisc-s-l384" bash scripts/gpu_prof.sh ${TAG}s > $UDM_OUT/prof_summary_${TAG}s.log 2>&1
bash scripts/gpu_pmc_bench.sh $TAG > $UDM_OUT/pmc_traffic_summary_$TAG.log 2>&1
bash scripts/gpu_pmc_mfma.sh $TAG > $UDM_OUT/pmc_mfma_summary_$TAG.log 2>&1
rm -rf $UDM_OUT/pmcb $UDM_OUT/pmcm $UDM_OUT/prof_$TAG $UDM_OUT/prof_${TAG}e $UDM_OUT/prof_${TAG}s
tail -4 $UDM_OUT/gputests_$TAG.log; cut -c1-400 $UDM_OUT/bench_1.4b_b8_$TAG.json; tail -3 $UDM_OUT/prof_summary_$TAG.log; tail -16 $UDM_OUT/pmc_traffic_summary_$TAG.log; tail -16 $UDM_OUT/pmc_mfma_summary_$TAG.log
python3 - <<'PY'
import json,glob
import os
for f in sorted(glob.glob(os.environ['UDM_OUT'] + '/bench_*_' + os.environ['TAG'] + '.json')):
    try:
        s=open(f).read(); j=json.loads(s[s.index('{'):])
        print(f, round(j['ms_per_step'],2), round(j['ms_per_step_median'],2), round(j['step_mfu'],4), round(j['roofline']['frac'],4))
    except Exception as e: print(f,'FAILED',e)
PY
