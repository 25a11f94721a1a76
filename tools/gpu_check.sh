#!/bin/bash
# Development helper: GPU parity tests, then the full bench line (headline, CPU baseline, extras).
# usage: OUT_DIR=<results directory> tools/gpu_check.sh <tag> [bench args]
tag=${1:-x}; shift
out=${OUT_DIR:?set OUT_DIR to the directory that receives the results}
mkdir -p "$out"
# a failed, faulted or timed-out step starts nothing further on the GPU
timeout -k 10 500 python -m pytest tests -m gpu -x -q > "$out/pytest_$tag.txt" 2>&1; rc=$?; echo "pytest rc=$rc"; tail -3 "$out/pytest_$tag.txt"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --steps 5 --warmup 2 --full "$@" > "$out/bench_$tag.json" 2> "$out/bench_$tag.err"; rc=$?; echo "bench rc=$rc"
[ $rc -eq 0 ] || exit $rc
python - <<PY
import json
d=json.load(open("$out/bench_$tag.json"))
print("value", d["value"], d["unit"], "ms/step", d["ms_per_step"])
print("stages", d["stages_ms"])
print("roofline", d["roofline"]["achieved"], d["roofline"]["frac"])
for k,v in d.get("extras",{}).items(): print(k, {a:b for a,b in v.items() if a not in ("note","roofline","cpu_baseline")})
print("parity", d.get("parity"))
PY
