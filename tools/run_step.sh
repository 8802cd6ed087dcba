#!/bin/bash
# tests of the convolution files + a 40-step fp32 bench line with its loss check ($OUT/bench_step.json; OUT defaults to out/)
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests/test_conv_gpu.py tests/test_chain_gpu.py -x -q > "$OUT"/t_step.log 2>&1; echo "rc=$?"; tail -3 "$OUT"/t_step.log
timeout -k 10 600 python bench.py --full --steps 40 --warmup 10 --no-cpu-baseline --no-other-configs > "$OUT"/bench_step.json 2> "$OUT"/bench_step.err; python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); print('step', round(d['ms_per_step'],3), round(d['median_ms_per_step'],3), d['loss_check']['worst_rel_err'])" "$OUT"/bench_step.json
