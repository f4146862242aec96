#!/usr/bin/env python3
"""ife_resample_bspline / ife_resample_bspline_f64 on one MI355X at the geometry of
scripts/bench_resample.py: 512 x 512 x 103 at (0.7, 0.7, 2.5) onto 512 x 512 x 412 at
(0.7, 0.7, 0.625), source and output resident in HBM, orders 3 and 5, float and double.  Prints one
JSON line and writes it to --out (default profiles/bspline.json).

  python scripts/bench_bspline.py [--steps 5] [--warmup 2] [--out profiles/bspline.json]

Per run, medians over --steps calls after --warmup calls, device time by a hipEvent pair on the
context's stream:
  prefilter  ife_bspline_coefficients* alone (the conversion to double and the three line passes,
             which is what the resampling call runs first); compulsory bytes: the source read once,
             the coefficients written once
  whole      the resampling call (prefilter, tables, gather)
  gather     whole - prefilter, a difference of two medians, not a measurement of its own;
             compulsory bytes: the coefficients read once, the output written once
each beside its compulsory bytes over its time and that rate as a fraction of the device-to-device
copy rate ife_measure_stream gives in the same run.  For information only: the linear ife_resample
call of the same run on the same data, and scipy (spline_filter + map_coordinates, mirror) on the
host on a volume an eighth the size along every axis."""
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

SRC_SHAPE, SRC_SPACING = (103, 512, 512), (0.7, 0.7, 2.5)
DST_SHAPE, DST_SPACING = (412, 512, 512), (0.7, 0.7, 0.625)
ORIGIN = (-179.2, -179.2, -300.0)
RUNS = [("float32_order%d" % o, np.float32, "F32", o) for o in (3, 5)] + \
       [("float64_order%d" % o, np.float64, None, o) for o in (3, 5)]


def median_ms(torch, call, steps, warmup):
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
    return statistics.median(times), min(times), max(times)


def rate(nbytes, ms, copy_gbs):
    gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else float("nan")
    return {"compulsory_bytes": nbytes, "GBs_vs_compulsory": round(gbs, 1),
            "fraction_of_measured_copy_rate": round(gbs / copy_gbs, 4)}


def measure(pkg, torch, ctx, name, dt, code, order, steps, warmup, copy_gbs):
    dev = torch.device("cuda", 0)
    src = (np.random.default_rng(7).standard_normal(SRC_SHAPE) * 1000).astype(dt)
    d_src = torch.from_numpy(src).to(dev)
    d_coef = torch.empty(SRC_SHAPE, dtype=torch.float64, device=dev)
    d_out = torch.empty(DST_SHAPE, dtype=getattr(torch, np.dtype(dt).name), device=dev)
    dtype = None if code is None else getattr(pkg, code)
    n_src, n_dst = int(np.prod(SRC_SHAPE)), int(np.prod(DST_SHAPE))

    pre = median_ms(torch, lambda: ctx.bspline_coefficients_device(d_src.data_ptr(), dtype, SRC_SHAPE, order,
                                                                   d_coef.data_ptr()), steps, warmup)
    whole = median_ms(torch, lambda: ctx.resample_bspline_device(
        d_src.data_ptr(), dtype, SRC_SHAPE, SRC_SPACING, ORIGIN, DST_SHAPE, DST_SPACING, ORIGIN, d_out.data_ptr(),
        order=order), steps, warmup)
    checksum = float(d_out[::37, ::41, ::43].double().sum().item())
    linear = median_ms(torch, lambda: ctx.resample_device(
        d_src.data_ptr(), dtype, SRC_SHAPE, SRC_SPACING, ORIGIN, DST_SHAPE, DST_SPACING, ORIGIN, d_out.data_ptr()),
        steps, warmup)
    gather_ms = whole[0] - pre[0]
    return {"run": name, "order": order,
            "prefilter": dict(median_ms=round(pre[0], 4), min_ms=round(pre[1], 4), max_ms=round(pre[2], 4),
                              **rate(src.nbytes + 8 * n_src, pre[0], copy_gbs)),
            "whole_call": dict(median_ms=round(whole[0], 4), min_ms=round(whole[1], 4), max_ms=round(whole[2], 4)),
            "gather_by_difference": dict(median_ms=round(gather_ms, 4),
                                         **rate(8 * n_src + n_dst * np.dtype(dt).itemsize, gather_ms, copy_gbs)),
            "linear_call_for_information_ms": round(linear[0], 4),
            "output_checksum": checksum}


def scipy_seconds(order):
    """scipy on the host, 64 x 64 x 13 -> 64 x 64 x 52 (information)"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    src = np.random.default_rng(7).standard_normal((13, 64, 64)) * 1000
    t0 = time.perf_counter()
    coef = ndimage.spline_filter(src, order, output=np.float64, mode="mirror")
    grid = np.meshgrid(np.arange(52) * 0.25, np.arange(64, dtype=np.float64), np.arange(64, dtype=np.float64),
                       indexing="ij")
    ndimage.map_coordinates(coef, grid, order=order, mode="mirror", prefilter=False)
    dt = time.perf_counter() - t0
    return {"order": order, "shape": [64, 64, 13], "onto": [64, 64, 52], "seconds": round(dt, 4),
            "Mvoxel_per_s": round(52 * 64 * 64 / dt / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bspline.json"))
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module(PKG)
    torch.cuda.set_device(0)
    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    nbytes = 1 << 30
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    copy_gbs = ctx.measure_stream(1, b.data_ptr(), a.data_ptr(), nbytes, 5)
    del a, b
    runs = [measure(pkg, torch, ctx, *r, args.steps, args.warmup, copy_gbs) for r in RUNS]
    out = {
        "metric": "ife_resample_bspline, 512x512x103 at (0.7, 0.7, 2.5) onto 512x512x412 at (0.7, 0.7, 0.625), "
                  "device resident",
        "value": runs[0]["whole_call"]["median_ms"], "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "data": "synthetic (seeded normal * 1000)",
        "measured_copy_GBs": round(copy_gbs, 1), "runs": runs,
        "scipy_on_the_host_for_information": [scipy_seconds(3), scipy_seconds(5)],
        "note": "one run, one box; nothing was tuned after it",
    }
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
