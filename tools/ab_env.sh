#!/bin/bash
# A/B of one environment switch on one box: tools/ab_env.sh VAR=a VAR=b -- bench args   (lines under $AB_OUT, default /tmp)
a="$1"; b="$2"; shift 3
out=${AB_OUT:-/tmp}
for round in 1 2; do
  for v in "$a" "$b"; do
    env "$v" python bench.py --full --no-extra --no-cpu-baseline "$@" > $out/abenv.json 2> $out/abenv.err
    python - "$v" "$out/abenv.json" <<'PY'
import json,sys
r=json.load(open(sys.argv[2])); s=r["stages"]
print(sys.argv[1], r["value"], "build", s["build_ms"], "acc", s["build_accumulate_ms"], "solve", s["fiedler_ms"], "mismatch", r["parity"]["w_cells_mismatched"])
PY
  done
done
