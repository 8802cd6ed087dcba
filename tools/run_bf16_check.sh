#!/bin/bash
# bf16 mode: its tests, a 40-step bench line (loss check, per-kernel times) and the per-launch table ($OUT/; OUT defaults to out/)
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests/test_bf16_gpu.py -x -q > "$OUT"/t_bf16.log 2>&1; echo "rc=$?"; tail -12 "$OUT"/t_bf16.log
timeout -k 10 600 python bench.py --full --precision bf16 --steps 40 --warmup 10 --no-cpu-baseline --no-other-configs > "$OUT"/bench_bf16.json 2> "$OUT"/bench_bf16.err; python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); print('bf16 step', round(d['ms_per_step'],3), round(d['median_ms_per_step'],3), d['loss_check']['worst_rel_err']); print({k:round(v,3) for k,v in sorted(d['kernels_ms_per_step'].items(), key=lambda kv:-kv[1])[:5]})" "$OUT"/bench_bf16.json
DVS_PRECISION=bf16 timeout -k 10 600 python tools/per_launch.py 12 4 4 > "$OUT"/per_launch_bf16.txt 2>&1; echo rc=$?
