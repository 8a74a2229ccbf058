#!/bin/bash
# On the GPU box: the full bench line (un-profiled, live PMC passes) and the rocprofv3 kernel traces of the same workloads.
# usage: tools/gpu_profile.sh <tag> <dir>     -> <dir>/bench_<tag>.json, pmc_<tag>.json, prof_<tag>[_encoder6|_rollout|_unet2x2]/
set -u
TAG=${1:-r03}
OUT=${2:?usage: tools/gpu_profile.sh <tag> <dir>}
export TMPDIR=/tmp
mkdir -p "$OUT"
rm -f "$OUT/pmc_$TAG.json"
python bench.py --full --pmc-out "$OUT/pmc_$TAG.json" > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err"
echo "bench rc=$?"
Q="--full --no-cpu-baseline --no-pmc --no-configs --no-roofline --no-dp-form --steps 60 --warmup 10 --blocks 2 --min-block-s 0.1"
rm -rf "$OUT/prof_$TAG" "$OUT/prof_${TAG}_encoder6" "$OUT/prof_${TAG}_rollout" "$OUT/prof_${TAG}_unet2x2"
timeout 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o r --output-format csv -- \
    python bench.py $Q > "$OUT/prof_$TAG.log" 2>&1
echo "rocprof unet2 rc=$?"
timeout 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof_${TAG}_encoder6" -o r --output-format csv -- \
    python bench.py $Q --no-companion --workload encoder6 --channels 7 --dtype f32 > "$OUT/prof_${TAG}_encoder6.log" 2>&1
echo "rocprof encoder6 rc=$?"
timeout 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof_${TAG}_rollout" -o r --output-format csv -- \
    python bench.py --no-cpu-baseline --no-pmc --no-configs --no-roofline --no-dp-form --no-companion --workload rollout --steps 6 --warmup 2 --blocks 2 --min-block-s 0.05 > "$OUT/prof_${TAG}_rollout.log" 2>&1
echo "rocprof rollout rc=$?"
timeout 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof_${TAG}_unet2x2" -o r --output-format csv -- \
    python bench.py $Q --no-companion --workload unet2x2 > "$OUT/prof_${TAG}_unet2x2.log" 2>&1
echo "rocprof unet2x2 rc=$?"
