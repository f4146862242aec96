#!/usr/bin/env python3
"""Differential features (ife_differential_features) on one MI355X: the synthetic volume and
two-ellipsoid mask of synthetic.py at 512^3, sigma = 1, 2, 4, everything resident in HBM, with
ife_emphysema_features (finite differences of the smoothed value) timed in the same run.  Prints
one JSON line and writes it to profiles/differential.json.

  python scripts/bench_differential.py [--size 512] [--sigmas 1 2 4] [--steps 5] [--warmup 1]

Per path: the median over --steps calls of the device time of one call over all scales (a hipEvent
pair on the context's stream, profiling off), then in a second loop with IFE_OPT_PROFILE on the
hipEvent time per kernel kind from inside the library, per call.  The jet kernel's achieved bytes
per second are against the 113 bytes per voxel it moves by design (twenty float fields and a mask
byte in, eight floats out), next to the copy rate of ife_measure_stream on the same box.

  python scripts/bench_differential.py --pipeline [--steps 5] [--warmup 1]

The consumers under IFE_OPT_DIFFERENTIAL, device resident, one process, written to
profiles/differential_pipeline.json: ife_samples_add_image (all-foreground branch, 512^3, sigma =
1, 2, 4, labels of the two ellipsoids) and ife_bag_dense_stream_begin up to the first _next (96^3,
box 15^3, 9 bins, sigma = 1: the configuration of profiles/dense_bag.json), each with the option at
0 and at 1, and for the option at 1 the composition of calls the fused kernels replace:
ife_differential_features into a planar volume, then ife_samples_add_features per scale, or
ife_dense_roi_histograms.  These calls block (a count comes back to the host), so the time is the
host clock around the call; the kernel times come from IFE_OPT_PROFILE in one further call."""
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
JET_BYTES_PER_VOXEL = 113
FIELD_PASSES = {"differential": 38, "finite_difference": 6}


def timed(torch, ctx, pkg, call, steps, warmup):
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
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4),
            "max_ms": round(max(times), 4),
            "kernel_ms_per_call": {k: round(t / steps, 4) for k, (c, t) in kt.items()},
            "kernel_launches_per_call": {k: c // steps for k, (c, t) in kt.items()}}


def spread(times):
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4),
            "max_ms": round(max(times), 4)}


def timed_blocking(pkg, ctx, call, steps, warmup):
    """Host-clock time of a call that blocks, then its kernel times from one profiled call."""
    import time
    for _ in range(warmup):
        call()
    times = []
    for _ in range(steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    ctx.set_option(pkg.OPT_PROFILE, 1)
    ctx.reset_kernel_times()
    call()
    kt = ctx.kernel_times()
    ctx.set_option(pkg.OPT_PROFILE, 0)
    r = spread(times)
    r["kernels"] = {k: {"launches": c, "total_ms": round(t, 4)} for k, (c, t) in kt.items()}
    return r


def pipeline(args):
    import ctypes as C
    import torch
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    lib = pkg.load_library()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    chk = ctx._chk
    fg = np.array([1, 2], np.uint32)

    def inputs(n):
        shape = (n, n, n)
        img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
        lab = synth.mask_ellipsoids(shape).astype(np.uint8)
        d_img, d_lab = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
        return shape, img, lab, d_img, d_lab, torch.clamp(d_lab, max=1)

    def features_planar(d_img, d_clamped, shape, sigmas, d_feat):
        ctx.differential_features_device(d_img.data_ptr(), pkg.F32, d_clamped.data_ptr(), pkg.U8, shape,
                                         (1.0, 1.0, 1.0), sigmas, d_feat.data_ptr(), layout=pkg.PLANAR)

    out = {"metric": "consumers of the differential feature path under IFE_OPT_DIFFERENTIAL, device resident",
           "unit": "ms", "higher_is_better": False, "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "data": "synthetic (volume_f32, two ellipsoids, unit spacing)",
           "trig_mode": int(os.environ.get("IFE_TRIG_MODE", "2"))}

    # ---- sample columns, all-foreground branch -----------------------------------------------------
    n, sigmas = args.size, args.sigmas
    shape, img, lab, d_img, d_lab, d_clamped = inputs(n)
    nvox, ns = n ** 3, len(sigmas)
    samples = ctx.samples(8 * ns)
    d = pkg._desc(shape, (1.0, 1.0, 1.0))
    sig = pkg._sigma_arg(sigmas)

    def add_image():
        samples.clear()
        chk(lib.ife_samples_add_image(ctx._h, samples._h, d_img.data_ptr(), pkg.F32, d_lab.data_ptr(), pkg.U8,
                                      C.byref(d), sig, ns, fg.ctypes.data, fg.size, None, 0, pkg.MEM_DEVICE))

    runs = {}
    for value in (0, 1):
        ctx.set_option(pkg.OPT_DIFFERENTIAL, value)
        runs["option_%d" % value] = timed_blocking(pkg, ctx, add_image, args.steps, args.warmup)
    ctx.set_option(pkg.OPT_DIFFERENTIAL, 0)
    d_feat = torch.empty((ns, 8) + shape, dtype=torch.float32, device=dev)

    def add_composed():
        samples.clear()
        features_planar(d_img, d_clamped, shape, sigmas, d_feat)
        for i in range(ns):
            chk(lib.ife_samples_add_features(ctx._h, samples._h, 8 * i, d_feat[i].data_ptr(), pkg.PLANAR, 8,
                                             d_lab.data_ptr(), pkg.U8, nvox, fg.ctypes.data, fg.size, None, 0,
                                             pkg.MEM_DEVICE))

    runs["composition"] = timed_blocking(pkg, ctx, add_composed, args.steps, args.warmup)
    out["samples_add_image"] = dict(runs, shape=list(shape), sigmas=sigmas, samples_per_column=samples.count(),
                                    foreground_fraction=round(float((lab != 0).mean()), 4))
    samples.close()
    del d_feat, d_img, d_lab, d_clamped, img, lab

    # ---- dense stream: _begin up to the first _next --------------------------------------------------
    n, size, bins, sigmas = 96, (15, 15, 15), 9, [1.0]
    shape, img, lab, d_img, d_lab, d_clamped = inputs(n)
    clamped = np.minimum(lab, 1)
    feat = ctx.differential_features(img, clamped, sigmas)[0]
    edges = np.stack([ctx.equalized_edges(ctx.sort_f32(feat[..., c][clamped != 0]), bins) for c in range(8)])
    edges = np.ascontiguousarray(edges, np.float32)
    d_edges = torch.from_numpy(edges).to(dev)
    d = pkg._desc(shape, (1.0, 1.0, 1.0))
    sig = pkg._sigma_arg(sigmas)
    box = pkg._size_arg(size)
    rows_host = {}

    def begin_to_first_next():
        nr, cap, row0, got = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        chk(lib.ife_bag_dense_stream_begin(ctx._h, d_img.data_ptr(), pkg.F32, d_lab.data_ptr(), pkg.U8, None, pkg.U8,
                                           C.byref(d), sig, 1, box, edges.ctypes.data, bins - 1, pkg.BAG_FREQUENCIES,
                                           0, C.byref(nr), C.byref(cap), pkg.MEM_DEVICE))
        if rows_host.get("cap", -1) < cap.value:
            rows_host["a"] = np.zeros((max(cap.value, 1), 8, bins), np.float32)
            rows_host["cap"] = cap.value
        chk(lib.ife_bag_dense_stream_next(ctx._h, rows_host["a"].ctypes.data, rows_host["a"].shape[0], C.byref(row0),
                                          C.byref(got)))
        rows_host["regions"] = nr.value

    def stream_call():
        begin_to_first_next()
        chk(lib.ife_bag_dense_stream_end(ctx._h))

    runs = {}
    for value in (0, 1):
        ctx.set_option(pkg.OPT_DIFFERENTIAL, value)
        runs["option_%d" % value] = timed_blocking(pkg, ctx, stream_call, args.steps, args.warmup)
    ctx.set_option(pkg.OPT_DIFFERENTIAL, 0)
    d_feat = torch.empty((8,) + shape, dtype=torch.float32, device=dev)
    d_counts = torch.empty((max(rows_host["regions"], 1), 8, bins), dtype=torch.int32, device=dev)

    def dense_composed():
        got = C.c_int64()
        features_planar(d_img, d_clamped, shape, sigmas, d_feat)
        chk(lib.ife_dense_roi_histograms(ctx._h, d_feat.data_ptr(), pkg.PLANAR, 8, d_clamped.data_ptr(), pkg.U8,
                                         d_lab.data_ptr(), pkg.U8, C.byref(d), box, d_edges.data_ptr(), bins - 1,
                                         d_counts.data_ptr(), d_counts.shape[0], C.byref(got), pkg.MEM_DEVICE))

    runs["composition"] = timed_blocking(pkg, ctx, dense_composed, args.steps, args.warmup)
    out["dense_stream_begin_to_first_next"] = dict(runs, shape=list(shape), box=list(size), bins=bins, sigmas=sigmas,
                                                   regions=rows_host["regions"],
                                                   note="option rows: _begin, the first _next (one block, frequencies "
                                                        "to the host) and _end; composition: counts left on the device")
    out["value"] = out["samples_add_image"]["option_1"]["median_ms"]
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sigmas", type=float, nargs="+", default=[1.0, 2.0, 4.0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pipeline", action="store_true",
                    help="time the sample and dense-stream calls under IFE_OPT_DIFFERENTIAL beside their composition")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles",
                                        "differential_pipeline.json" if args.pipeline else "differential.json")
    if args.pipeline:
        return pipeline(args)
    import torch
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = args.size
    shape, spacing, ns = (n, n, n), (1.0, 1.0, 1.0), len(args.sigmas)
    nvox = n ** 3
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    d_img, d_mask = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    d_out = torch.empty((ns,) + shape + (8,), dtype=torch.float32, device=dev)

    def differential():
        ctx.differential_features_device(d_img.data_ptr(), pkg.F32, d_mask.data_ptr(), pkg.U8, shape, spacing,
                                         args.sigmas, d_out.data_ptr())

    def finite_difference():
        ctx.emphysema_features_device(d_img.data_ptr(), pkg.F32, d_mask.data_ptr(), pkg.U8, shape, spacing,
                                      args.sigmas, d_out.data_ptr())

    runs = {"finite_difference": timed(torch, ctx, pkg, finite_difference, args.steps, args.warmup),
            "differential": timed(torch, ctx, pkg, differential, args.steps, args.warmup)}
    for name, r in runs.items():
        r["field_passes_per_scale"] = FIELD_PASSES[name]
        r["ms_per_scale"] = round(r["median_ms"] / ns, 4)
    del d_out
    nbytes = 4 << 30
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    copy_gbs = ctx.measure_stream(1, b.data_ptr(), a.data_ptr(), nbytes, 5)
    jet_ms = runs["differential"]["kernel_ms_per_call"]["jet_features"] / ns
    jet_gbs = JET_BYTES_PER_VOXEL * nvox / (jet_ms * 1e-3) / 1e9
    out = {
        "metric": "differential features, float32 volume + uint8 mask -> 8 features per scale, device resident",
        "value": runs["differential"]["median_ms"], "unit": "ms", "higher_is_better": False, "n_gpus": 1,
        "shape": [n, n, n], "sigmas": args.sigmas, "steps": args.steps, "warmup": args.warmup,
        "data": "synthetic (volume_f32, two ellipsoids, unit spacing)",
        "foreground_fraction": round(float(mask.mean()), 4),
        "trig_mode": int(os.environ.get("IFE_TRIG_MODE", "2")),
        "runs": runs,
        "cost_ratio_per_scale": round(runs["differential"]["median_ms"] / runs["finite_difference"]["median_ms"], 3),
        "jet_kernel": {"ms_per_scale": round(jet_ms, 4), "bytes_per_voxel": JET_BYTES_PER_VOXEL,
                       "achieved_GBs": round(jet_gbs, 1), "measured_copy_GBs": round(copy_gbs, 1),
                       "frac_of_measured_copy": round(jet_gbs / copy_gbs, 4),
                       "frac_of_hbm_peak": round(jet_gbs / HBM_PEAK_GBS, 4)},
        "hbm_peak_GBs": HBM_PEAK_GBS,
    }
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
