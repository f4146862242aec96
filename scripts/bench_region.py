#!/usr/bin/env python3
"""The three region calls on one MI355X, device resident, one configuration: the bounding box of
a uint8 mask (ife_mask_bounding_box), the float crop to that box (ife_extract_region) and the
membership of a uint16 label map in a set of three values (ife_label_membership).

  python scripts/bench_region.py [--size 512] [--steps 5] [--warmup 2] [--out profiles/region.json]

Input: the two-ellipsoid mask of synthetic.py; the image is random floats made on the device (a
copy of bits does not care), the label map is the mask's labels spread over uint16.  Every call
blocks, so a call is timed on the host clock: the median of --steps calls after --warmup; the
hipEvent time of the call's kernel (IFE_OPT_PROFILE) is recorded beside it.  Each time is set
against the bytes the call cannot avoid moving and against the copy rate ife_measure_stream
reaches in the same run.  The results are compared with torch's on the device.  Writes the result
to --out and prints it as one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region.json"))
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    import torch

    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    shape = (args.size,) * 3
    nvox = args.size ** 3
    labels = synth.mask_ellipsoids(shape)
    mask = np.minimum(labels, 1).astype(np.uint8)
    include = [300, 600, 65535]
    lab16 = (labels.astype(np.uint16) * 300)
    lab16[::7, ::5, ::3] = 65535
    d_mask = torch.from_numpy(mask).cuda()
    d_lab = torch.from_numpy(lab16.view(np.int16)).cuda()   # torch has no uint16 arithmetic: bits only
    d_img = torch.rand(shape, dtype=torch.float32, device="cuda")
    d_member = torch.empty(shape, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()

    # the copy rate of this run: 256 MiB, read and written once per pass
    sbytes = 256 << 20
    d_a = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    copy_gbs = ctx.measure_stream(1, d_b.data_ptr(), d_a.data_ptr(), sbytes, reps=5)   # bytes read + written
    del d_a, d_b

    box = {}

    def do_box():
        box["v"] = ctx.mask_bounding_box_device(d_mask.data_ptr(), pkg.U8, shape)

    t_box = timed(do_box, args.steps, args.warmup)
    index, size, count = box["v"]
    d_crop = torch.full(tuple(size[::-1]), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def do_crop():
        ctx.extract_region_device(d_img.data_ptr(), 4, shape, index, size, d_crop.data_ptr())

    def do_member():
        ctx.label_membership_device(d_lab.data_ptr(), pkg.U16, nvox, include, d_member.data_ptr(), inside=1, outside=0)

    t_crop = timed(do_crop, args.steps, args.warmup)
    t_member = timed(do_member, args.steps, args.warmup)

    # the same results from torch
    spans = []
    for axes in ((0, 1), (0, 2), (1, 2)):   # x, y, z
        hit = torch.nonzero(d_mask.amax(dim=axes)).flatten()
        spans.append((int(hit[0]), int(hit[-1]) - int(hit[0]) + 1))
    want_box = (tuple(s[0] for s in spans), tuple(s[1] for s in spans), int(d_mask.count_nonzero()))
    (x0, y0, z0), (sx, sy, sz) = index, size
    crop_equal = bool(torch.equal(d_crop, d_img[z0:z0 + sz, y0:y0 + sy, x0:x0 + sx]))
    want_member = torch.isin(d_lab, torch.tensor(np.array(include, np.uint16).view(np.int16), device="cuda"))
    member_equal = bool(torch.equal(d_member, want_member.to(torch.int16)))
    box_equal = want_box == (index, size, count)

    def entry(times, nbytes, kernels):
        ms = statistics.median(times)
        kms = sum(kernels.values())
        return {"ms": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
                "compulsory_bytes": int(nbytes), "gb_per_s": round(nbytes / ms / 1e6, 1),
                "of_copy_rate": round(nbytes / ms / 1e6 / copy_gbs, 3),
                "kernel_ms": kernels, "kernel_gb_per_s": round(nbytes / kms / 1e6, 1) if kms else None,
                "kernel_of_copy_rate": round(nbytes / kms / 1e6 / copy_gbs, 3) if kms else None}

    crop_vox = sx * sy * sz
    out = {
        "metric": "region calls, device resident: bounding box of a uint8 mask, float crop to it, membership of a "
                  "uint16 label map in three values; each against its compulsory bytes and the copy rate of the run",
        "value": round(statistics.median(t_box) + statistics.median(t_crop) + statistics.median(t_member), 4),
        "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "shape": list(shape), "steps": args.steps, "warmup": args.warmup,
        "data": "synthetic (two-ellipsoid mask, random float image, labels spread over uint16)",
        "copy_rate_gb_per_s": round(copy_gbs, 1), "copy_bytes": sbytes,
        "box": {"index": list(index), "size": list(size), "count": int(count),
                "kept_fraction": round(crop_vox / nvox, 4)},
        "bounding_box": entry(t_box, nvox, kernel_ms(pkg, ctx, do_box)),
        "crop": entry(t_crop, 2 * 4 * crop_vox, kernel_ms(pkg, ctx, do_crop)),
        "membership": entry(t_member, 2 * 2 * nvox, kernel_ms(pkg, ctx, do_member)),
        "include": include,
        "results_equal": {"bounding_box": box_equal, "crop": crop_equal, "membership": member_equal},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not (box_equal and crop_equal and member_equal):
        sys.exit("a region result differs from torch's")


if __name__ == "__main__":
    main()
