#!/bin/bash
# 300 timed steps of the headline workload (with its loss check) + a repeat of the deterministic-repeat check ($OUT/; OUT defaults to out/)
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full --steps 300 --warmup 10 --no-cpu-baseline --no-other-configs --no-stock-caller > "$OUT"/bench_soak.json 2> "$OUT"/bench_soak.err; python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); print('soak: step', round(d['ms_per_step'],3), round(d['median_ms_per_step'],3), d['loss_check'])" "$OUT"/bench_soak.json
timeout -k 10 600 python tools/repeat_check.py > "$OUT"/repeat_check.txt 2>&1; echo "repeat rc=$?"; tail -5 "$OUT"/repeat_check.txt
