#!/usr/bin/env python3
"""The census and coverage calls on one MI355X, device resident, one configuration: the value
census of a float volume (ife_value_census_f32) beside the sort alone (ife_sort_f32), the
threshold to a byte mask (ife_threshold_mask), and the coverage of a mask by 2000 boxes of
53 x 53 x 41 in the twelve cumulative rounds of ImageBrowser (ife_roi_coverage).

  python scripts/bench_coverage.py [--size 512] [--steps 5] [--warmup 2] [--out profiles/coverage.json]

Input: the synthetic volume of synthetic.py truncated to CT numbers (a few thousand distinct values,
what the census is asked of) as floats, and its two-ellipsoid mask clamped to {0, 1}; the boxes are
ife_random_rois' on that mask.  Every call blocks, so a call is timed on the host clock: the median
of --steps calls after --warmup; the hipEvent time of the call's kernels (IFE_OPT_PROFILE) is
recorded beside it.  Beside each call stand its compulsory bytes against the copy rate
ife_measure_stream reaches in the same run, and beside the coverage call the hipMemcpy of the mask
to pageable host memory, which is what a caller with a device-resident mask pays today before any
host count could begin.  No speed is required: the script fails only where a result differs from
the definitions restated in numpy (tests/coverage_oracle.py).  Writes the result to --out and
prints it as one JSON line."""
import argparse
import ctypes as C
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
HIP_MEMCPY_DEVICE_TO_HOST = 2


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def kernel_ms(pkg, ctx, fn):
    """hipEvent time of the kernels of one call, by kind"""
    ctx.set_option(pkg.OPT_PROFILE, 1)
    ctx.reset_kernel_times()
    fn()
    out = {name: round(ms, 4) for name, (n, ms) in ctx.kernel_times().items() if n}
    ctx.set_option(pkg.OPT_PROFILE, 0)
    return out


def hip_runtime():
    """The HIP runtime this process already runs on (torch's or the system's), for hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in os.path.basename(path):
            lib = C.CDLL(path)
            lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return lib
    sys.exit("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage.json"))
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    import coverage_oracle as V
    import torch

    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    shape = (args.size,) * 3
    nvox = args.size ** 3
    box = (53, 53, 41) if args.size >= 64 else (5, 5, 3)
    ends, seed = V.ROUND_ENDS, 2024
    n_boxes = ends[-1]
    low, high = -950.0, -700.0
    image = synth.volume_i16(shape, synth.SEED_CONFIG[3]).astype(np.float32)
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    d_img = torch.from_numpy(image).cuda()
    d_mask = torch.from_numpy(mask).cuda()
    d_thr = torch.zeros(nvox, dtype=torch.uint8, device="cuda")
    d_sorted = torch.zeros(nvox, dtype=torch.float32, device="cuda")
    d_rois = torch.zeros(n_boxes * 6, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    # the copy rate of this run: 256 MiB, read and written once per pass
    sbytes = 256 << 20
    d_a = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    copy_gbs = ctx.measure_stream(1, d_b.data_ptr(), d_a.data_ptr(), sbytes, reps=5)   # bytes read + written
    del d_a, d_b

    hip = hip_runtime()
    host = np.zeros(nvox, np.uint8)   # written once, so that its pages exist

    def do_memcpy():
        if hip.hipMemcpy(host.ctypes.data, d_mask.data_ptr(), nvox, HIP_MEMCPY_DEVICE_TO_HOST) != 0:
            sys.exit("hipMemcpy failed")

    got = {}
    got["n"] = ctx.value_census_device(d_img.data_ptr(), nvox)
    n_unique = got["n"][0]
    d_uniq = torch.zeros(max(n_unique, 1), dtype=torch.float32, device="cuda")
    d_counts = torch.zeros(max(n_unique, 1), dtype=torch.int32, device="cuda")
    ctx.random_rois_device(d_mask.data_ptr(), pkg.U8, shape, d_rois.data_ptr(), n_boxes, size=box, seed=seed)

    def do_census():
        got["census"] = ctx.value_census_device(d_img.data_ptr(), nvox, d_uniq.data_ptr(), d_counts.data_ptr(), n_unique)

    def do_sort():
        ctx.sort_f32_device(d_img.data_ptr(), nvox, d_sorted.data_ptr())
        ctx.synchronize()   # the sort alone does not wait on device memory; the census does

    def do_threshold():
        got["threshold"] = ctx.threshold_mask_device(d_img.data_ptr(), nvox, low, high, d_thr.data_ptr())

    def do_coverage():
        got["coverage"] = ctx.roi_coverage_device(d_mask.data_ptr(), pkg.U8, shape, d_rois.data_ptr(), n_boxes, ends)

    t_memcpy = timed(do_memcpy, args.steps, args.warmup)
    t_census = timed(do_census, args.steps, args.warmup)
    t_sort = timed(do_sort, args.steps, args.warmup)
    t_threshold = timed(do_threshold, args.steps, args.warmup)
    t_coverage = timed(do_coverage, args.steps, args.warmup)

    # the results against the definitions
    uniq, counts, n_nan = V.value_census(image)
    census_equal = bool(got["census"] == (uniq.size, n_nan)
                        and np.array_equal(d_uniq.cpu().numpy().view(np.uint32)[:uniq.size], uniq.view(np.uint32))
                        and np.array_equal(d_counts.cpu().numpy().view(np.uint32)[:uniq.size], counts))
    want_mask, want_count = V.threshold_mask(image, low, high)
    threshold_equal = bool(got["threshold"] == want_count
                           and np.array_equal(d_thr.cpu().numpy(), want_mask.reshape(-1)))
    rois = d_rois.cpu().numpy().reshape(n_boxes, 6)
    visited, hits, region = V.roi_coverage(mask, rois, ends)
    coverage_equal = bool(np.array_equal(got["coverage"][0], visited) and np.array_equal(got["coverage"][1], hits)
                          and got["coverage"][2] == region)

    def entry(times, kernels, nbytes):
        ms = statistics.median(times)
        kms = sum(kernels.values())
        return {"ms": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
                "kernel_ms": kernels, "compulsory_bytes": int(nbytes), "gb_per_s": round(nbytes / ms / 1e6, 1),
                "of_copy_rate": round(nbytes / ms / 1e6 / copy_gbs, 3),
                "kernel_gb_per_s": round(nbytes / kms / 1e6, 1) if kms else None,
                "kernel_of_copy_rate": round(nbytes / kms / 1e6 / copy_gbs, 3) if kms else None}

    ms_cov, ms_memcpy = statistics.median(t_coverage), statistics.median(t_memcpy)
    plane_bytes = 4 * ((nvox + 31) // 32)
    out = {
        "metric": "census and coverage calls, device resident: ife_roi_coverage of 2000 boxes in twelve rounds "
                  "against the hipMemcpy of the mask to pageable host memory that a host count needs first",
        "value": round(ms_cov, 4), "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "shape": list(shape), "steps": args.steps, "warmup": args.warmup,
        "data": "synthetic (volume truncated to CT numbers as float32, two-ellipsoid mask clamped to {0, 1})",
        "box": list(box), "n_boxes": n_boxes, "round_ends": list(ends), "seed": seed,
        "thresholds": [low, high], "n_unique": int(n_unique), "n_nan": int(got["n"][1]),
        "region_size": int(region), "visited": [int(v) for v in visited], "hits": [int(v) for v in hits],
        "copy_rate_gb_per_s": round(copy_gbs, 1), "copy_bytes": sbytes,
        "memcpy_to_pageable_host": {"ms": round(ms_memcpy, 4), "ms_min": round(min(t_memcpy), 4),
                                    "ms_max": round(max(t_memcpy), 4), "bytes": nvox,
                                    "gb_per_s": round(nvox / ms_memcpy / 1e6, 2)},
        # the array read once; the outputs are a few kilobytes
        "value_census": entry(t_census, kernel_ms(pkg, ctx, do_census), 4 * nvox),
        "sort_alone": entry(t_sort, kernel_ms(pkg, ctx, do_sort), 2 * 4 * nvox),
        # the image read, the mask written
        "threshold_mask": entry(t_threshold, kernel_ms(pkg, ctx, do_threshold), 5 * nvox),
        # the mask read once, its plane written, and per round both planes read
        "roi_coverage": entry(t_coverage, kernel_ms(pkg, ctx, do_coverage),
                              nvox + plane_bytes + len(set(ends)) * 2 * plane_bytes),
        "census_of_sort": round(statistics.median(t_census) / statistics.median(t_sort), 3),
        "roi_coverage_of_memcpy": round(ms_cov / ms_memcpy, 4),
        "results_equal": {"value_census": census_equal, "threshold_mask": threshold_equal,
                          "roi_coverage": coverage_equal, "memcpy": bool(np.array_equal(host, mask.ravel()))},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not all(out["results_equal"].values()):
        sys.exit("a result differs from the definition")


if __name__ == "__main__":
    main()
