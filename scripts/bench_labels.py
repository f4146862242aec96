#!/usr/bin/env python3
"""The labels of one dense bag on one MI355X: the sliding form (ife_dense_roi_labels) against the
box list (ife_roi_labels on the boxes of the same generator), same process, device-resident
inputs and output.

  python scripts/bench_labels.py [--size 96] [--box 15] [--steps 5] [--warmup 2]
                                 [--out profiles/labels.json]

Input: the dense-bag bench configuration (scripts/bench_dense_bag.py): the two-ellipsoid labels
of synthetic.py as the generating mask, a label volume of three labels in slabs along x.  Both
calls block, so a call is timed on the host clock.  The two label arrays must be equal to each
other and to the numpy oracle (tests/labels_oracle.py) on a sample of the regions, whose rate is
recorded for information.  Then the hipEvent time per kernel kind of one call of each
(IFE_OPT_PROFILE).  Writes the result to --out and prints it as one JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
PKG = "image-feature-extraction_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--box", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-sample", type=int, default=2000, help="regions the numpy oracle is timed and compared on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labels.json"))
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    import torch
    import labels_oracle
    from bench_dense_bag import dense_boxes, kernel_ms, spread, timed

    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    lib = pkg.load_library()
    shape, size = (args.size,) * 3, (args.box,) * 3
    gen = synth.mask_ellipsoids(shape).astype(np.uint8)
    lab = np.zeros(shape, np.uint8)
    lab[:, :, args.size // 3:] = 1
    lab[:, :, 2 * args.size // 3:] = 2
    boxes = dense_boxes(gen, size)
    n = len(boxes)
    d = pkg._desc(shape, (1.0, 1.0, 1.0))
    d_lab, d_gen = torch.from_numpy(lab).cuda(), torch.from_numpy(gen).cuda()
    d_boxes = torch.from_numpy(boxes).cuda()
    d_dense = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    d_list = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def check(rc):
        if rc:
            sys.exit("call failed: %d %s" % (rc, lib.ife_last_error(ctx._h).decode()))

    def dense():
        got = C.c_int64()
        check(lib.ife_dense_roi_labels(ctx._h, d_lab.data_ptr(), pkg.U8, d_gen.data_ptr(), pkg.U8, C.byref(d),
                                       pkg._size_arg(size), None, 0, -1, d_dense.data_ptr(), n, C.byref(got),
                                       pkg.MEM_DEVICE))
        return got.value

    def listed():
        check(lib.ife_roi_labels(ctx._h, d_lab.data_ptr(), pkg.U8, C.byref(d), d_boxes.data_ptr(), n, None, 0, -1,
                                 d_list.data_ptr(), pkg.MEM_DEVICE))
        return n

    got_n, t_dense = timed(dense, args.steps, args.warmup)
    _, t_list = timed(listed, args.steps, args.warmup)
    a, b = d_dense.cpu().numpy(), d_list.cpu().numpy()
    pick = np.linspace(0, n - 1, min(args.oracle_sample, n)).astype(np.int64)
    t0 = time.perf_counter()
    ref = labels_oracle.roi_labels(lab, boxes[pick])
    t_oracle = time.perf_counter() - t0
    equal = bool(got_n == n and np.array_equal(a, b) and np.array_equal(a[pick], ref))
    ms_dense, ms_list = statistics.median(t_dense), statistics.median(t_list)
    out = {
        "metric": "labels of one dense bag: ife_roi_labels on the box list over ife_dense_roi_labels, "
                  "device-resident inputs and output",
        "value": round(ms_list / ms_dense, 2), "unit": "x", "higher_is_better": True, "n_gpus": 1,
        "shape": list(shape), "box": list(size), "labels": [int(v) for v in np.unique(lab)], "regions": int(n),
        "steps": args.steps, "warmup": args.warmup,
        "data": "synthetic (two ellipsoids generate, three label slabs along x)",
        "dense_ms": spread(t_dense), "list_ms": spread(t_list),
        "dense_regions_per_s": round(n / ms_dense * 1e3), "list_regions_per_s": round(n / ms_list * 1e3),
        "numpy_oracle_regions_per_s": round(len(pick) / t_oracle), "numpy_oracle_regions": int(len(pick)),
        "labels_equal": equal,
        "dense_kernels": kernel_ms(pkg, ctx, dense), "list_kernels": kernel_ms(pkg, ctx, listed),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not equal:
        sys.exit("the dense labels differ from those of the box list or the oracle")


if __name__ == "__main__":
    main()
