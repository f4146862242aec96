#!/usr/bin/env python3
"""Signed Maurer distance map (ife_signed_distance_map) on one MI355X: the two-ellipsoid mask of
synthetic.py at 256^3 and 512^3, mask and map resident in HBM.  Prints one JSON line.

  python scripts/bench_distance.py [--sizes 256 512] [--steps 5] [--warmup 1]

Per size: the median over --steps calls of the device time of one call (a hipEvent pair on the
context's stream, profiling off), then in a second loop with IFE_OPT_PROFILE on the hipEvent time
per kernel kind from inside the library.  GB/s is against the compulsory 9 bytes per voxel (the
mask read once, the float64 map written once); what the three passes move by design is given
beside it.  The last field compares the y and z kernels at the two largest sizes: 8 per doubling
of the edge is linear work per line, 16 would be quadratic."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "image-feature-extraction_amd"
HBM_PEAK_GBS = 8000.0


def measure(pkg, synth, torch, ctx, n, steps, warmup):
    shape = (n, n, n)
    dev = torch.device("cuda", 0)
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    d_mask = torch.from_numpy(mask).to(dev)
    d_out = torch.empty(shape, dtype=torch.float64, device=dev)

    def call():
        ctx.signed_distance_map_device(d_mask.data_ptr(), pkg.U8, shape, (1.0, 1.0, 1.0), d_out.data_ptr())

    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ctx.set_option(pkg.OPT_PROFILE, 1)
    ctx.reset_kernel_times()
    for _ in range(steps):
        call()
    kt = ctx.kernel_times()
    ctx.set_option(pkg.OPT_PROFILE, 0)
    nvox = n ** 3
    ms = statistics.median(times)
    inside = d_out[d_mask != 0]
    res = {
        "shape": [n, n, n], "foreground_fraction": round(float(mask.mean()), 4),
        "median_ms": round(ms, 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
        "kernel_ms": {k: round(t / c, 4) for k, (c, t) in kt.items()},
        "compulsory_bytes": 9 * nvox,
        "GBs_vs_compulsory_9B_per_voxel": round(9 * nvox / (ms * 1e-3) / 1e9, 1),
        "frac_of_hbm_peak": round(9 * nvox / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        # x: mask in, map out; y and z: map in and out, a 12-byte stack entry written per site
        # kept and read back on the walk (at most one per voxel)
        "moved_bytes_by_design_upper": (9 + 2 * (16 + 24)) * nvox + nvox,
        "max_inside_distance": float(inside.max()) if inside.numel() else None,
    }
    del d_mask, d_out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    torch.cuda.set_device(0)
    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    runs = [measure(pkg, synth, torch, ctx, n, args.steps, args.warmup) for n in sorted(args.sizes)]
    out = {
        "metric": "signed Maurer distance map, uint8 mask -> float64 map, device resident",
        "value": runs[-1]["median_ms"], "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "data": "synthetic (two ellipsoids, unit spacing)",
        "hbm_peak_GBs": HBM_PEAK_GBS, "runs": runs,
    }
    if len(runs) >= 2 and runs[-1]["shape"][0] == 2 * runs[-2]["shape"][0]:
        small, big = runs[-2]["kernel_ms"], runs[-1]["kernel_ms"]
        ratios = {k: round(big[k] / small[k], 2) for k in ("edt_x", "edt_y", "edt_z") if small.get(k)}
        yz = (big["edt_y"] + big["edt_z"]) / (small["edt_y"] + small["edt_z"])
        out["scaling_%d_over_%d" % (runs[-1]["shape"][0], runs[-2]["shape"][0])] = {
            "per_kernel": ratios, "y_plus_z": round(yz, 2),
            "nearer_8_linear_than_16_quadratic": bool(abs(yz - 8.0) < abs(yz - 16.0))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
