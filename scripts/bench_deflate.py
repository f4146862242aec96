#!/usr/bin/env python3
"""DEFLATE on the device (ife_deflate) on one MI355X, written to profiles/deflate.json.

  python scripts/bench_deflate.py [--size 512] [--steps 5] [--warmup 1]

One process, the GaussianBlur and Eigenvalue1 planes of the two-ellipsoid volume of synthetic.py at
sigma = 1 (planar ife_emphysema_features, device resident).  Per plane, the median of --steps
behind --warmup: ife_deflate device to device (host clock around the blocking call, in ms and in
input GB/s), a hipMemcpy of the raw plane to pageable host memory, zlib.compress(plane, 1) on the
host with its size beside the device's, and once the copy rate of ife_measure_stream.

  python scripts/bench_deflate.py --tool [--size 256] [--rounds 3]

ExtractFeatures wall time on a volume of --size^3 with three scales, with and without
IFE_DEVICE_GZIP=1, alternating, --rounds rounds; merged into the same file under "tool".

The bars are against what the same run measures: the device call must take less time than the
raw plane's copy to the host (otherwise it only saves CPU time), and the tool must be faster
with the variable in every round.  The size relative to zlib level 1 carries no bar."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "image-feature-extraction_amd"
PLANES = {"GaussianBlur": 0, "Eigenvalue1": 2}


def median_ms(call, steps, warmup):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4),
            "max_ms": round(max(times), 4)}


def merge_out(path, update):
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out.update(update)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(update), flush=True)


def planes(args):
    import torch
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    n = args.size
    shape = (n, n, n)
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    d_img, d_mask = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    d_feat = torch.empty((1, 8) + shape, dtype=torch.float32, device=dev)
    ctx.emphysema_features_device(d_img.data_ptr(), pkg.F32, d_mask.data_ptr(), pkg.U8, shape, (1.0, 1.0, 1.0),
                                  [1.0], d_feat.data_ptr(), layout=pkg.PLANAR)
    ctx.synchronize()
    nbytes = 4 * n ** 3
    cap = ctx.deflate_bound(nbytes)
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    host = np.empty(nbytes, np.uint8)
    result = {}
    for name, comp in PLANES.items():
        print("plane %s" % name, file=sys.stderr, flush=True)
        plane = d_feat[0, comp]
        got = {}

        def device_call():
            got["n"], got["crc"] = ctx.deflate_device(plane.data_ptr(), nbytes, d_out.data_ptr(), cap)

        dd = median_ms(device_call, args.steps, args.warmup)
        dd["input_GBs"] = round(nbytes / (dd["median_ms"] * 1e-3) / 1e9, 1)

        def raw_copy():
            pkg_hip_copy(torch, host, plane)

        cp = median_ms(raw_copy, args.steps, args.warmup)
        raw = host.tobytes()
        assert got["crc"] == zlib.crc32(raw)
        z = {}

        def host_zlib():
            z["n"] = len(zlib.compress(raw, 1))

        hz = median_ms(host_zlib, min(args.steps, 3), 0)
        result[name] = {"plane_bytes": nbytes, "ife_deflate_device_to_device": dd, "raw_copy_to_host": cp,
                        "host_zlib_level_1": hz, "device_bytes": got["n"], "zlib_level_1_bytes": z["n"],
                        "device_over_zlib_size": round(got["n"] / z["n"], 4),
                        "device_ratio": round(got["n"] / nbytes, 4),
                        "bar_device_call_faster_than_raw_copy": dd["median_ms"] < cp["median_ms"]}
    del d_feat
    a = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    b = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    copy_gbs = ctx.measure_stream(1, b.data_ptr(), a.data_ptr(), 1 << 30, 5)
    merge_out(args.out, {"metric": "ife_deflate of one float32 feature plane, device to device",
                         "unit": "ms", "higher_is_better": False, "n_gpus": 1, "shape": [n, n, n], "sigma": 1.0,
                         "steps": args.steps, "warmup": args.warmup,
                         "data": "synthetic (volume_f32, two ellipsoids, unit spacing)",
                         "foreground_fraction": round(float(mask.mean()), 4),
                         "value": result["GaussianBlur"]["ife_deflate_device_to_device"]["median_ms"],
                         "measured_copy_GBs": round(copy_gbs, 1), "planes": result})


def pkg_hip_copy(torch, host, plane):
    """The raw plane to pageable host memory, blocking."""
    torch.from_numpy(host).view(torch.float32).copy_(plane.reshape(-1))
    torch.cuda.synchronize()


def tool(args):
    import niftiio
    synth = importlib.import_module(PKG + ".synthetic")
    n = args.size
    shape = (n, n, n)
    exe = os.path.join(ROOT, PKG, "host", "bin", "ExtractFeatures")
    rounds = []
    with tempfile.TemporaryDirectory() as tmp:
        niftiio.write(os.path.join(tmp, "i.nii.gz"), synth.volume_f32(shape, synth.SEED_CONFIG[3]))
        niftiio.write(os.path.join(tmp, "m.nii.gz"), np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8))
        for r in range(args.rounds):
            row = {}
            for label, value in (("host_zlib", None), ("device_gzip", "1")):
                env = dict(os.environ)
                env.pop("IFE_DEVICE_GZIP", None)
                env.pop("IFE_DEVICES", None)
                if value:
                    env["IFE_DEVICE_GZIP"] = value
                t0 = time.perf_counter()
                subprocess.check_call([exe, "-i", os.path.join(tmp, "i.nii.gz"), "-m", os.path.join(tmp, "m.nii.gz"),
                                       "-o", os.path.join(tmp, "o_%s_%d" % (label, r)), "-s", "1", "-s", "2", "-s",
                                       "4"], env=env)
                row[label + "_s"] = round(time.perf_counter() - t0, 3)
                row[label + "_bytes"] = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp)
                                            if f.startswith("o_%s_%d" % (label, r)))
            row["bar_device_gzip_faster"] = row["device_gzip_s"] < row["host_zlib_s"]
            print("round %d: %s" % (r, row), file=sys.stderr, flush=True)
            rounds.append(row)
    merge_out(args.out, {"tool": {"what": "ExtractFeatures wall time, three scales, 24 .nii.gz files",
                                  "shape": [n, n, n], "sigmas": [1.0, 2.0, 4.0], "rounds": rounds,
                                  "bar_device_gzip_faster_in_every_round":
                                      all(r["bar_device_gzip_faster"] for r in rounds)}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tool", action="store_true", help="time ExtractFeatures with and without IFE_DEVICE_GZIP=1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate.json"))
    args = ap.parse_args()
    args.size = args.size or (256 if args.tool else 512)
    return tool(args) if args.tool else planes(args)


if __name__ == "__main__":
    main()
