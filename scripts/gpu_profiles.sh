#!/bin/bash
# rocprofv3 kernel-trace stats + the two PMC passes for each named config (scripts/profile_round.sh), then the full bench line
# usage: OUT_DIR=<dir> scripts/gpu_profiles.sh <tag> <config>...
tag=${1:-r03}; shift
out=${OUT_DIR:?set OUT_DIR to the directory for the logs and the bench line}
mkdir -p "$out"
for cfg in "$@"; do
  timeout -k 10 ${PROF_TIMEOUT:-330} bash scripts/profile_round.sh $tag $cfg > "$out/${tag}_prof_${cfg}.log" 2>&1 || { echo "profile $cfg failed"; tail -5 "$out/${tag}_prof_${cfg}.log"; exit 1; }
  echo "profile $cfg done"
done
timeout -k 10 400 python bench.py --full > "$out/${tag}_bench_default.json" 2> "$out/${tag}_bench_default.err"
tail -c 500 "$out/${tag}_bench_default.json"
