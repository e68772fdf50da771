#!/bin/bash
# the driver's command with --full, then a digest of its line: tools/r04/bench_run.sh [bench.py args]; the line and the
# log go to $BENCH_OUT (default bench_out/)
cd "$(dirname "$0")/../.."; O=${BENCH_OUT:-bench_out}; mkdir -p "$O"
timeout -k 10 900 python bench.py --full "$@" > "$O/bench_default.json" 2> "$O/bench_default.err"; echo "bench rc=$?"; tail -3 "$O/bench_default.err"
python - "$O/bench_default.json" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print("headline", d["ms_per_step"], d["infer"]["ms_per_step"], d["dtype"][:40], d["roofline"])
print("conv", d["conv_kernels"])
print("dice", d["dice"])
print("cpu", {k: v for k, v in d.get("cpu_baseline", {}).items() if k != "sample"})
for k in ("cfg3","fp32_mfma"):
    e=d.get(k)
    if e: print(k, e["ms_per_step"], e["infer_ms"], e["roofline"]["frac"], e["roofline"]["kernel"], e.get("max_abs_diff_of_step0_probabilities_vs_headline"), e["final_loss"], d["final_loss"])
PY
