#!/usr/bin/env python3
"""ife_scale_select on one MI355X, device resident, one configuration: four measures (Laplacian,
tube, plate, blob; bright, gamma 1) over sigma = 1, 2, 4 of a 512^3 volume, beside
ife_emphysema_features (PLANAR, device resident) of the same scales in the same process, which is
the yardstick: the selection runs the same feature launches into a one-scale workspace and folds
each scale into its outputs.

  python scripts/bench_scale_select.py [--size 512] [--steps 5] [--warmup 2] [--out profiles/scale_select.json]

Input: the synthetic volume of synthetic.py and its two-ellipsoid mask clamped to {0, 1}.  Every
call blocks, so a call is timed on the host clock: the median of --steps calls after --warmup.  The
fold kernel alone is the `mask_f64` row of the kernel-time table (IFE_OPT_PROFILE; no other kernel
of the call is booked there), read against its compulsory bytes -- four feature planes read and
5 M bytes written per voxel and scale, 5 M more read from the second scale on -- and the copy rate
ife_measure_stream reaches in the same run.  No speed is required: the script fails only where the
Laplacian row differs from the same fold formed with torch from the yardstick's features (one float
product per scale, exact).  The measurement runs in a child process under a time limit of its own;
the parent never opens the device.  Writes the result to --out and prints it as one JSON line."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "image-feature-extraction_amd"
SIGMAS = [1.0, 2.0, 4.0]


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


def measure(args):
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    import torch

    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    shape = (args.size,) * 3
    nvox = args.size ** 3
    S = len(SIGMAS)
    image = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    d_img = torch.from_numpy(image).cuda()
    d_mask = torch.from_numpy(mask).cuda()
    del image

    # the copy rate of this run: 256 MiB, read and written once per pass
    sbytes = 256 << 20
    d_a = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    copy_gbs = ctx.measure_stream(1, d_b.data_ptr(), d_a.data_ptr(), sbytes, reps=5)   # bytes read + written
    del d_a, d_b

    d_feat = torch.empty((S, 8, nvox), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def do_features():
        ctx.emphysema_features_device(d_img.data_ptr(), pkg.F32, d_mask.data_ptr(), pkg.U8, shape, (1.0, 1.0, 1.0),
                                      SIGMAS, d_feat.data_ptr(), layout=pkg.PLANAR)
        ctx.synchronize()   # the DEVICE feature call only enqueues; the selection blocks

    t_features = timed(do_features, args.steps, args.warmup)
    k_features = kernel_ms(pkg, ctx, do_features)
    # c as the tests choose it: the median over scales and foreground of sigma^2 * Frobenius norm
    fg = d_mask.reshape(-1) != 0
    c = float(torch.cat([float(s) ** 2 * d_feat[k, 7][fg] for k, s in enumerate(SIGMAS)]).median().item())
    measures = [pkg.ScaleMeasure(pkg.SS_LAPLACIAN, 1, 1.0)] + [pkg.ScaleMeasure(k, 1, 1.0, 0.5, 0.5, c)
                                                              for k in (pkg.SS_TUBE, pkg.SS_PLATE, pkg.SS_BLOB)]
    M = len(measures)
    # the Laplacian row from the yardstick's features: one float product per scale, exact
    best = torch.zeros(nvox, dtype=torch.float32, device="cuda")
    at = torch.full((nvox,), 255, dtype=torch.uint8, device="cuda")
    for k, s in enumerate(SIGMAS):
        w = float(np.float32(float(np.float32(s)) ** 2.0))
        r = -(d_feat[k, 5] * w)
        wins = r > best
        best = torch.where(wins, r, best)
        at[wins] = k
    del d_feat, r, wins
    torch.cuda.empty_cache()

    d_resp = torch.empty((M, nvox), dtype=torch.float32, device="cuda")
    d_idx = torch.empty((M, nvox), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def do_select():
        ctx.scale_select_device(d_img.data_ptr(), pkg.F32, d_mask.data_ptr(), pkg.U8, shape, (1.0, 1.0, 1.0), SIGMAS,
                                measures, d_resp.data_ptr(), d_idx.data_ptr())

    t_select = timed(do_select, args.steps, args.warmup)
    k_select = kernel_ms(pkg, ctx, do_select)
    laplacian_equal = bool(torch.equal(d_resp[0].view(torch.int32), best.view(torch.int32)) and torch.equal(d_idx[0], at))
    chosen = [[int((d_idx[m] == k).sum().item()) for k in range(S)] for m in range(M)]

    fold_ms = k_select.get("mask_f64", 0.0)
    fold_bytes = nvox * (S * 16 + S * 5 * M + (S - 1) * 5 * M)
    ms_sel, ms_feat = statistics.median(t_select), statistics.median(t_features)
    out = {
        "metric": "ife_scale_select, four measures over three scales, device resident, beside ife_emphysema_features "
                  "(PLANAR, device resident) of the same scales in the same process",
        "value": round(ms_sel, 4), "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "shape": list(shape), "sigmas": SIGMAS, "steps": args.steps, "warmup": args.warmup,
        "data": "synthetic (float32 volume, two-ellipsoid mask clamped to {0, 1})",
        "measures": ["laplacian", "tube", "plate", "blob"], "polarity": 1, "gamma": 1.0, "alpha": 0.5, "beta": 0.5,
        "c": c,
        "copy_rate_gb_per_s": round(copy_gbs, 1), "copy_bytes": sbytes,
        "scale_select": {"ms": round(ms_sel, 4), "ms_min": round(min(t_select), 4), "ms_max": round(max(t_select), 4),
                         "kernel_ms": k_select, "output_bytes": 5 * M * nvox},
        "emphysema_features_planar": {"ms": round(ms_feat, 4), "ms_min": round(min(t_features), 4),
                                      "ms_max": round(max(t_features), 4), "kernel_ms": k_features,
                                      "output_bytes": 32 * S * nvox},
        "scale_select_of_features": round(ms_sel / ms_feat, 4),
        "fold": {"kernel_ms": fold_ms, "launches": S, "compulsory_bytes": int(fold_bytes),
                 "gb_per_s": round(fold_bytes / fold_ms / 1e6, 1) if fold_ms else None,
                 "of_copy_rate": round(fold_bytes / fold_ms / 1e6 / copy_gbs, 3) if fold_ms else None,
                 # what folding inside the feature kernel would save: the scale written and read once
                 "round_trip_bytes": int(2 * 32 * S * nvox)},
        "voxels_per_chosen_scale": chosen,
        "results_equal": {"laplacian_row": laplacian_equal},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not all(out["results_equal"].values()):
        sys.exit("a result differs from the definition")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_select.json"))
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return measure(args)
    # the GPU step runs in a child under its own time limit; nothing follows it on the device
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker",
           "--size", str(args.size), "--steps", str(args.steps), "--warmup", str(args.warmup), "--out", args.out]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
