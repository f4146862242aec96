#!/usr/bin/env python3
"""The differential feature path over the Z-slab engine: two measurements, one process, written to
profiles/multi_differential.json (one run on one box; medians of --steps after --warmup).

  python scripts/bench_multi_differential.py [--size 512] [--sigmas 1 2 4] [--steps 5] [--warmup 1]

1. The lean sweep in its two forms (ife_stage_z_sweep_order).  One slab of 512 x 512 x 64 with its
   overlap planes, sigma = 2, the six Z jobs of one scale (cT and c at the orders 0, 1, 2), all
   lines, a neighbour on the incoming side -- the sweep as it sits on the chain from device to
   device.  Source-major job order takes the shared-read kernels (every plane loaded once for its
   three orders), interleaved order the per-job kernels; causal and anticausal.  The time is the
   library's own hipEvent pair around the launches of a call (IFE_OPT_PROFILE, row zslab_sweep);
   the two forms alternate call by call.

2. The whole call from host memory to host memory: the synthetic volume and two-ellipsoid mask at
   --size^3, Context.differential_features against Multi.differential_features on the device list
   [0] and [0, 0, 0, 0], host clock around the blocking call.  With one GPU the last two show what
   the slab schedule COSTS (uploads with overlap, chains, per-slab launches on one device), not a
   speed-up.  With several GPUs the distinct device lists of 2, 4 and 8 are timed too; otherwise
   the file says that more than one distinct device is unmeasured."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "image-feature-extraction_amd"


def spread(times):
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4),
            "max_ms": round(max(times), 4)}


def lean_sweeps(pkg, torch, dev, steps, warmup):
    nz, ny, nx, sigma = 64, 512, 512, 2.0
    shape, L = (nz, ny, nx), ny * nx
    lo, hi = pkg.Z_OVERLAP_LO, pkg.Z_OVERLAP_HI
    ctx = pkg.Context(0)
    gen = torch.Generator(device=dev).manual_seed(7)
    ext = [torch.rand((lo + nz + hi, ny, nx), generator=gen, dtype=torch.float32, device=dev) for _ in range(2)]
    src = [e[lo:lo + nz] for e in ext]   # views: data_ptr() is the slab's plane 0
    cks = [torch.zeros(ctx.stage_z_ck_bytes(shape), dtype=torch.uint8, device=dev) for _ in range(6)]
    sin = torch.rand(6 * 4 * L, generator=gen, dtype=torch.float64, device=dev)
    sout = torch.zeros(6 * 4 * L, dtype=torch.float64, device=dev)
    forms = {"shared_read": [(s, k) for s in range(2) for k in range(3)],     # source-major
             "per_job": [(s, k) for k in range(3) for s in range(2)]}         # interleaved
    ctx.set_option(pkg.OPT_PROFILE, 1)

    def call(direction, form):
        jobs = forms[form]
        ctx.reset_kernel_times()
        ctx.stage_z_sweep_order(direction, [src[s].data_ptr() for s, k in jobs], shape, (1.0, 1.0, 1.0), 0, L,
                                [sigma] * 6, [k for s, k in jobs], True, sin.data_ptr(), sout.data_ptr(),
                                [cks[3 * s + k].data_ptr() for s, k in jobs])
        ctx.synchronize()
        return ctx.kernel_times()["zslab_sweep"][1]

    out = {"slab": [nz, ny, nx], "sigma": sigma, "jobs": 6, "lines": L, "neighbour": True,
           "timer": "IFE_OPT_PROFILE, row zslab_sweep: device time of the launches of one call"}
    for direction, name in ((0, "causal"), (1, "anticausal")):
        times = {f: [] for f in forms}
        for i in range(warmup + steps):
            for f in forms:   # alternating
                t = call(direction, f)
                if i >= warmup:
                    times[f].append(t)
        out[name] = {f: spread(t) for f, t in times.items()}
        out[name]["shared_over_per_job"] = round(out[name]["shared_read"]["median_ms"] /
                                                 out[name]["per_job"]["median_ms"], 4)
    ctx.close()
    return out


def whole_call(pkg, synth, torch, size, sigmas, steps, warmup):
    shape, spacing = (size, size, size), (1.0, 1.0, 1.0)
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)

    def timed(call):
        times, result = [], None
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            result = call()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                times.append(dt)
        return spread(times), result

    out = {"shape": list(shape), "sigmas": sigmas, "memory": "host in, host out (pageable numpy arrays)",
           "timer": "host clock around the blocking call", "runs": {}}
    print("whole call: context", file=sys.stderr, flush=True)
    with pkg.Context(0) as c:
        out["runs"]["context"], ref = timed(lambda: c.differential_features(img, mask, sigmas, spacing))
    ref = ref.view(np.uint32)
    lists = {"multi_1x_device0": [0], "multi_4x_device0": [0] * 4}
    ngpu = torch.cuda.device_count()
    for n in (2, 4, 8):
        if n <= ngpu:
            lists["multi_%d_distinct" % n] = list(range(n))
    for name, devices in lists.items():
        print("whole call: %s" % name, file=sys.stderr, flush=True)
        with pkg.Multi(devices) as m:
            out["runs"][name], got = timed(lambda: m.differential_features(img, mask, sigmas, spacing))
        out["runs"][name]["devices"] = devices
        out["runs"][name]["equals_context_bit_for_bit"] = bool(np.array_equal(got.view(np.uint32), ref))
        del got
    out["gpus_on_the_box"] = ngpu
    if ngpu < 2:
        out["unmeasured"] = "more than one distinct device: the box has one GPU"
    out["note"] = ("a device listed several times runs the whole slab schedule on one GPU: these rows show what "
                   "the schedule costs, not a speed-up")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sigmas", type=float, nargs="+", default=[1.0, 2.0, 4.0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_differential.json"))
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    torch.cuda.set_device(0)   # raises when there is no device: no number without a GPU
    dev = torch.device("cuda", 0)
    out = {"metric": "differential features over the Z-slab engine", "unit": "ms", "higher_is_better": False,
           "steps": args.steps, "warmup": args.warmup, "statistic": "median of the timed calls",
           "scope": "one run on one box",
           "trig_mode": int(os.environ.get("IFE_TRIG_MODE", "2")),
           "lean_sweep": lean_sweeps(pkg, torch, dev, args.steps, args.warmup)}
    torch.cuda.empty_cache()
    out["whole_call"] = whole_call(pkg, synth, torch, args.size, args.sigmas, args.steps, args.warmup)
    out["value"] = out["whole_call"]["runs"]["multi_4x_device0"]["median_ms"]
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
