#!/usr/bin/env python3
"""ife_resample / ife_resample_f64 on one MI355X in the Resample tool's stated use, a volume from
one reconstruction thickness onto another: 512 x 512 x 103 at (0.7, 0.7, 2.5) onto 512 x 512 x 412
at (0.7, 0.7, 0.625), source and output resident in HBM.  Prints one JSON line and writes it to
--out (default profiles/resample.json).

  python scripts/bench_resample.py [--steps 5] [--warmup 2] [--out profiles/resample.json]

Per run (float -> float linear, double -> double linear, uint8 -> uint8 nearest): the median over
--steps calls of the device time of one call (a hipEvent pair on the context's stream; the call
builds and uploads its axis tables inside that window), the compulsory bytes (the source read
once, the output written once) over that time, and that rate as a fraction of the device-to-device
copy rate ife_measure_stream gives in the same run.  For information only: the numpy oracle's time
on a volume an eighth the size along every axis."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "image-feature-extraction_amd"

SRC_SHAPE, SRC_SPACING = (103, 512, 512), (0.7, 0.7, 2.5)
DST_SHAPE, DST_SPACING = (412, 512, 512), (0.7, 0.7, 0.625)
ORIGIN = (-179.2, -179.2, -300.0)
RUNS = (("float32_linear", np.float32, "F32", 0, np.float32),
        ("float64_linear", np.float64, None, 0, np.float64),
        ("uint8_nearest", np.uint8, "U8", 1, np.uint8))


def measure(pkg, torch, ctx, name, sdt, code, interp, odt, steps, warmup, copy_gbs):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    src = (rng.integers(0, 3, SRC_SHAPE).astype(sdt) if sdt == np.uint8
           else rng.standard_normal(SRC_SHAPE).astype(sdt))
    d_src = torch.from_numpy(src).to(dev)
    d_out = torch.empty(DST_SHAPE, dtype=getattr(torch, np.dtype(odt).name), device=dev)
    dtype = None if code is None else getattr(pkg, code)

    def call():
        ctx.resample_device(d_src.data_ptr(), dtype, SRC_SHAPE, SRC_SPACING, ORIGIN, DST_SHAPE, DST_SPACING,
                            ORIGIN, d_out.data_ptr(), interpolation=interp)

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
    ms = statistics.median(times)
    nbytes = src.nbytes + int(np.prod(DST_SHAPE)) * np.dtype(odt).itemsize
    gbs = nbytes / (ms * 1e-3) / 1e9
    return {"run": name, "median_ms": round(ms, 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
            "compulsory_bytes": nbytes, "GBs_vs_compulsory": round(gbs, 1),
            "fraction_of_measured_copy_rate": round(gbs / copy_gbs, 4),
            "output_checksum": float(d_out[::37, ::41, ::43].double().sum().item())}


def oracle_seconds():
    """the numpy definition on 64 x 64 x 13 -> 64 x 64 x 52 (information)"""
    import resample_oracle as R
    src = np.random.default_rng(7).standard_normal((13, 64, 64))
    t0 = time.perf_counter()
    R.resample(src, SRC_SPACING, ORIGIN, (52, 64, 64), DST_SPACING, ORIGIN)
    dt = time.perf_counter() - t0
    return {"shape": [64, 64, 13], "onto": [64, 64, 52], "seconds": round(dt, 4),
            "Mvoxel_per_s": round(52 * 64 * 64 / dt / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
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
        "metric": "ife_resample, 512x512x103 at (0.7, 0.7, 2.5) onto 512x512x412 at (0.7, 0.7, 0.625), device resident",
        "value": runs[0]["median_ms"], "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "data": "synthetic (seeded normal / labels 0..2)",
        "measured_copy_GBs": round(copy_gbs, 1), "runs": runs,
        "numpy_oracle_for_information": oracle_seconds(),
        "note": "measured once, one box",
    }
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
