#!/usr/bin/env python3
"""A/B of two builds of libife_hip.so on one box: bench.py, interleaved, round by round.

    python3 scripts/experiments/slp_ab.py --parent scripts/experiments/libs/parent.so \
        [--change image-feature-extraction_amd/csrc/libife_hip.so] [--rounds 3] [--out profiles/slp_ab.json]

Every bench run is a fresh process under its own time limit, selected by IFE_HIP_LIB; the order
inside a round alternates (parent first, change first, ...), so a drift of the box does not fall
on one side.  Written: the step and the kernel table (avg ms per launch) of every run, the
parent's own spread over the rounds (max - min), and whether the change beats the parent by
more than that spread in every round.  The first failing run ends the script.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(lib, steps, warmup, limit):
    env = dict(os.environ, IFE_HIP_LIB=os.path.abspath(lib))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       stdin=subprocess.DEVNULL, text=True, timeout=limit, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        raise SystemExit("bench.py with %s ended with status %d" % (lib, p.returncode))
    line = [ln for ln in p.stdout.splitlines() if ln.lstrip().startswith("{")][-1]
    d = json.loads(line)
    return {"ms_per_step": d["ms_per_step"],
            "kernels_avg_ms": {k: v["avg_ms"] for k, v in d["roofline"]["kernels"].items()},
            "kernels_ms_per_step": {k: v["ms_per_step"] for k, v in d["roofline"]["kernels"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--change", default=os.path.join(ROOT, "image-feature-extraction_amd", "csrc", "libife_hip.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per bench run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slp_ab.json"))
    a = ap.parse_args()
    rounds = []
    for r in range(a.rounds):
        order = ("parent", "change") if r % 2 == 0 else ("change", "parent")
        res = {"order": list(order)}
        for side in order:
            res[side] = bench(a.parent if side == "parent" else a.change, a.steps, a.warmup, a.limit)
            print("round %d %-6s %.3f ms  %s" % (r + 1, side, res[side]["ms_per_step"],
                                                 res[side]["kernels_avg_ms"]), flush=True)
        rounds.append(res)
    steps_p = [r["parent"]["ms_per_step"] for r in rounds]
    steps_c = [r["change"]["ms_per_step"] for r in rounds]
    spread = max(steps_p) - min(steps_p)
    kernels = {}
    for k in rounds[0]["parent"]["kernels_avg_ms"]:
        kp = [r["parent"]["kernels_avg_ms"][k] for r in rounds]
        kc = [r["change"]["kernels_avg_ms"].get(k) for r in rounds]
        ks = max(kp) - min(kp)
        kernels[k] = {"parent": kp, "change": kc, "parent_spread_ms": round(ks, 4),
                      "slower_beyond_spread": bool(min(c - p for c, p in zip(kc, kp)) > ks
                                                   or sum(kc) / len(kc) - sum(kp) / len(kp) > ks),
                      "faster_beyond_spread_every_round": bool(all(p - c > ks for c, p in zip(kc, kp)))}
    doc = {"what": "bench.py --gpus 1 --steps %d --warmup %d, parent and change interleaved on one box, "
                   "fresh process per run; avg ms per launch from the bench line's kernel table"
                   % (a.steps, a.warmup),
           "parent_lib": os.path.relpath(os.path.abspath(a.parent), ROOT),
           "change_lib": os.path.relpath(os.path.abspath(a.change), ROOT),
           "rounds": rounds,
           "step_ms": {"parent": steps_p, "change": steps_c, "parent_spread_ms": round(spread, 4),
                       "margin_ms_each_round": [round(p - c, 4) for p, c in zip(steps_p, steps_c)],
                       "faster_beyond_spread_every_round": bool(all(p - c > spread for p, c in zip(steps_p, steps_c)))},
           "kernels_avg_ms": kernels}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["step_ms"]))
    print({k: (v["slower_beyond_spread"], v["faster_beyond_spread_every_round"]) for k, v in kernels.items()})


if __name__ == "__main__":
    main()
