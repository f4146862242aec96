#!/usr/bin/env python3
"""The blocking calls of the one-process multi-device engine from host memory to host memory:
Multi.differential_features and Multi.emphysema_features at --size^3, sigmas 1 2 4, on the device
lists [0] and [0, 0, 0, 0], host clock around the blocking call (the loop of whole_call in
scripts/bench_multi_differential.py).  Prints one JSON line with every timed step; the library is
the tree's own or the one IFE_HIP_LIB names, so that two builds can be timed in turn
(profiles/multi_phases_ab.json).  With one GPU the figures show the host and schedule cost of the
engine, not a speed-up; more than one distinct device is not measured here.

  [IFE_HIP_LIB=/path/to/libife_hip.so] python scripts/bench_multi_calls.py [--steps 5] [--warmup 1] [--label NAME]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "image-feature-extraction_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    shape, spacing, sigmas = (args.size,) * 3, (1.0, 1.0, 1.0), [1.0, 2.0, 4.0]
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    out = {"label": args.label, "lib": pkg.LIB_PATH, "shape": list(shape), "sigmas": sigmas, "runs": {}}
    for name, devices in (("1x_device0", [0]), ("4x_device0", [0, 0, 0, 0])):
        with pkg.Multi(devices) as m:
            for call in ("differential_features", "emphysema_features"):
                f = getattr(m, call)
                times, crc = [], None
                for i in range(args.warmup + args.steps):
                    t0 = time.perf_counter()
                    got = f(img, mask, sigmas, spacing)
                    dt = (time.perf_counter() - t0) * 1e3
                    if i >= args.warmup:
                        times.append(round(dt, 3))
                    if i == 0:   # a fingerprint of the result, compared between the libraries
                        crc = int(np.bitwise_xor.reduce(got.view(np.uint32).ravel()[::97]))
                    del got
                out["runs"]["%s %s" % (call, name)] = {"steps_ms": times, "xor_every_97th_word": crc}
                print("%s %s %s: %s" % (args.label, call, name, times), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
