#!/bin/bash
# End-of-round check on the GPU box: full `-m gpu` suite, the bench with every leg (--full), smoke ($OUT/; OUT defaults to out/)
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"
timeout -k 10 1100 python -m pytest tests -m gpu -x -q > "$OUT"/final_pytest_gpu.log 2>&1; echo "pytest rc=$?"; tail -3 "$OUT"/final_pytest_gpu.log
T0=$(date +%s)
timeout -k 10 1100 python bench.py --full > "$OUT"/final_bench_default.json 2> "$OUT"/final_bench_default.err; echo "bench rc=$? wall=$(( $(date +%s) - T0 ))s"
python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); print(d['value'], d['ms_per_step'], d['median_ms_per_step']); print(d['roofline']['frac'], d['roofline_chain']['chain_bwd_kernel']['ms_per_step']); print(d['stock_caller']['ms_per_step'], d['cpu_baseline']['value']); print({k:(v.get('ms_per_step'), v.get('value')) for k,v in d['other_configs'].items()})" "$OUT"/final_bench_default.json
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/final_smoke.log 2>&1; tail -3 "$OUT"/final_smoke.log
