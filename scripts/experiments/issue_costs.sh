#!/bin/bash
# Runs issue_probe (built beside it if missing) at 1, 2, 3, 4 and 6 waves per SIMD, every step
# under its own time limit, and merges the five objects into profiles/issue_costs.json (or $1).
# The chain stops at the first step that fails.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
out=${1:-$root/profiles/issue_costs.json}
probe=$here/issue_probe
[ -x "$probe" ] || /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -o "$probe" "$here/issue_probe.hip"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
for w in 1 2 3 4 6; do
  timeout -k 10 120 "$probe" $w > "$tmp/w$w.json"
done
python3 - "$out" "$tmp"/w1.json "$tmp"/w2.json "$tmp"/w3.json "$tmp"/w4.json "$tmp"/w6.json <<'EOF'
import json, sys
runs = [json.load(open(p)) for p in sys.argv[2:]]
doc = {"what": "cycles per wave64 vector instruction and SIMD (scripts/experiments/issue_probe.hip): "
               "launch time x the clock held in that launch / (waves per SIMD x instructions per wave)",
       "device": runs[0]["device"], "arch": runs[0]["arch"], "cus": runs[0]["cus"],
       "insts_per_wave": runs[0]["insts_per_wave"],
       "by_waves_per_simd": {str(r["waves_per_simd"]): r["classes"] for r in runs}}
json.dump(doc, open(sys.argv[1], "w"), indent=1)
open(sys.argv[1], "a").write("\n")
EOF
echo "wrote $out"
