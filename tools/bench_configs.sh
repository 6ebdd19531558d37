#!/bin/bash
# The SURVEY §8 d workloads C2..C5 on one GPU (C2 = the driver's line); one JSON line each,
# written to $OUT (default: bench_out/).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
for c in ${CONFIGS:-C2 C3 C4 C5}; do
  timeout -k 10 600 python bench.py --full --config $c --steps ${STEPS:-5} --warmup 2 --no-cpu-baseline --all-kernels > $OUT/bench_$c.json 2> $OUT/bench_$c.err || { tail -5 $OUT/bench_$c.err; exit 1; }
  python - "$OUT/bench_$c.json" "$c" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(sys.argv[2], d["metric"], "|", d["value"], "cw/s", d["ms_per_step"], "ms", d["config"]["kernel"],
      "| e2e", d["e2e_with_rng"]["codewords_per_s"], "| others", d.get("kernels"), "| FER", d["fer_at_snr"]["fer_last"])
PY
done
