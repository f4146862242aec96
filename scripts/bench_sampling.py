#!/usr/bin/env python3
"""The sampling calls on one MI355X, device resident, one configuration: the count of the
admissible voxels of a uint8 mask (ife_sample_positions without draws), 50 boxes of 53 x 53 x 41
(ife_random_rois), 10^6 positions (ife_sample_positions) and the gather of those 50 boxes from a
float volume (ife_extract_rois).

  python scripts/bench_sampling.py [--size 512] [--steps 5] [--warmup 2] [--out profiles/sampling.json]

Input: the two-ellipsoid mask of synthetic.py, clamped to {0, 1}; the image is random floats made
on the device (a copy of bits does not care).  Every call blocks, so a call is timed on the host
clock: the median of --steps calls after --warmup; the hipEvent time of the call's kernels
(IFE_OPT_PROFILE) is recorded beside it.  The count pass is set against the copy rate
ife_measure_stream reaches in the same run.  The bar: the 50-box call takes less than a hipMemcpy
of the mask to pageable host memory, which is what a caller with a device-resident mask pays before
the host generator can start; the script fails where it does not.  The 50 boxes are compared with
the definition restated in numpy (tests/sampling_oracle.py).  Writes the result to --out and prints
it as one JSON line."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling.json"))
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    import sampling_oracle as S
    import torch

    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    shape = (args.size,) * 3
    nvox = args.size ** 3
    box = (53, 53, 41) if args.size >= 64 else (5, 5, 3)
    n_boxes, n_positions, seed = 50, 10 ** 6, 2024
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    d_mask = torch.from_numpy(mask).cuda()
    d_img = torch.rand(shape, dtype=torch.float32, device="cuda")
    d_rois = torch.zeros(n_boxes * 6, dtype=torch.int64, device="cuda")
    d_pos = torch.zeros(n_positions, dtype=torch.int64, device="cuda")
    d_out = torch.full((n_boxes,) + box[::-1], float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    # the copy rate of this run: 256 MiB, read and written once per pass
    sbytes = 256 << 20
    d_a = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    copy_gbs = ctx.measure_stream(1, d_b.data_ptr(), d_a.data_ptr(), sbytes, reps=5)   # bytes read + written
    del d_a, d_b

    # what a device-resident caller pays today: the mask to pageable host memory
    hip = hip_runtime()
    host = np.zeros(nvox, np.uint8)   # written once, so that its pages exist

    def do_memcpy():
        if hip.hipMemcpy(host.ctypes.data, d_mask.data_ptr(), nvox, HIP_MEMCPY_DEVICE_TO_HOST) != 0:
            sys.exit("hipMemcpy failed")

    counts = {}

    def do_count():
        counts["v"] = ctx.sample_positions_device(d_mask.data_ptr(), pkg.U8, shape, None, 0, size=box)

    def do_rois():
        ctx.random_rois_device(d_mask.data_ptr(), pkg.U8, shape, d_rois.data_ptr(), n_boxes, size=box, seed=seed)

    def do_positions():
        ctx.sample_positions_device(d_mask.data_ptr(), pkg.U8, shape, d_pos.data_ptr(), n_positions, seed=seed)

    def do_gather():
        ctx.extract_rois_device(d_img.data_ptr(), 4, shape, d_rois.data_ptr(), n_boxes, d_out.data_ptr())

    t_memcpy = timed(do_memcpy, args.steps, args.warmup)
    t_count = timed(do_count, args.steps, args.warmup)
    t_rois = timed(do_rois, args.steps, args.warmup)
    t_pos = timed(do_positions, args.steps, args.warmup)
    t_gather = timed(do_gather, args.steps, args.warmup)

    # the results against the definition
    want, want_counts = S.random_rois(mask, n_boxes, box, seed=seed)
    rois = d_rois.cpu().numpy().reshape(n_boxes, 6)
    rois_equal = bool(np.array_equal(rois, want[0]) and int(counts["v"][0]) == int(want_counts[0]))
    memcpy_equal = bool(np.array_equal(host, mask.ravel()))
    pos = d_pos.cpu().numpy()
    fg = np.flatnonzero(mask.ravel())
    pos_equal = bool(np.array_equal(pos[:200], [fg[S.rank(seed, 0, k, len(fg))] for k in range(200)])
                     and (mask.ravel()[pos] != 0).all())
    gather_equal = all(bool(torch.equal(d_out[i], d_img[z:z + box[2], y:y + box[1], x:x + box[0]]))
                       for i, (x, y, z) in enumerate(rois[:, :3].tolist()))

    def entry(times, kernels, nbytes=None):
        ms = statistics.median(times)
        e = {"ms": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "kernel_ms": kernels}
        if nbytes is not None:
            kms = sum(kernels.values())
            e.update({"compulsory_bytes": int(nbytes), "gb_per_s": round(nbytes / ms / 1e6, 1),
                      "of_copy_rate": round(nbytes / ms / 1e6 / copy_gbs, 3),
                      "kernel_gb_per_s": round(nbytes / kms / 1e6, 1) if kms else None,
                      "kernel_of_copy_rate": round(nbytes / kms / 1e6 / copy_gbs, 3) if kms else None})
        return e

    ms_rois, ms_memcpy = statistics.median(t_rois), statistics.median(t_memcpy)
    out = {
        "metric": "sampling calls, device-resident uint8 mask: 50 seeded boxes (ife_random_rois) against the "
                  "hipMemcpy of the mask to pageable host memory that the host generator needs first",
        "value": round(ms_rois, 4), "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "shape": list(shape), "steps": args.steps, "warmup": args.warmup,
        "data": "synthetic (two-ellipsoid mask clamped to {0, 1}, random float image)",
        "box": list(box), "n_boxes": n_boxes, "n_positions": n_positions, "seed": seed,
        "n_admissible": int(counts["v"][0]), "foreground": int(fg.size),
        "copy_rate_gb_per_s": round(copy_gbs, 1), "copy_bytes": sbytes,
        "memcpy_to_pageable_host": {"ms": round(ms_memcpy, 4), "ms_min": round(min(t_memcpy), 4),
                                    "ms_max": round(max(t_memcpy), 4), "bytes": nvox,
                                    "gb_per_s": round(nvox / ms_memcpy / 1e6, 2)},
        "count": entry(t_count, kernel_ms(pkg, ctx, do_count), nvox),
        "random_rois": entry(t_rois, kernel_ms(pkg, ctx, do_rois)),
        "sample_positions": entry(t_pos, kernel_ms(pkg, ctx, do_positions)),
        "extract_rois": entry(t_gather, kernel_ms(pkg, ctx, do_gather), 2 * 4 * n_boxes * box[0] * box[1] * box[2]),
        "random_rois_of_memcpy": round(ms_rois / ms_memcpy, 4),
        "bar_met": bool(ms_rois < ms_memcpy),
        "results_equal": {"random_rois": rois_equal, "sample_positions": pos_equal, "extract_rois": gather_equal,
                          "memcpy": memcpy_equal},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not all(out["results_equal"].values()):
        sys.exit("a sampling result differs from the definition")
    if not out["bar_met"]:
        sys.exit("the 50-box call took longer than the copy of the mask to the host")


if __name__ == "__main__":
    main()
