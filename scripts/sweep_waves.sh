#!/bin/bash
# sweep the number of persistent wavefronts of the work-queue kernels (bench.py --waves); usage: OUT_DIR=<dir> scripts/sweep_waves.sh
out=${OUT_DIR:?set OUT_DIR to the directory for the bench lines}
mkdir -p "$out"
for w in 512 1024 2048 4096; do
  python bench.py --full --steps 10 --warmup 2 --cpu-sample 0 --waves $w 2>> "$out/bench_err.log" > "$out/sweep_$w.json"
  python -c "import json; d=json.load(open('$out/sweep_$w.json')); print($w, d['value'], d['ms_per_step'], d['roofline']['kernel_ms_per_step'])"
done
