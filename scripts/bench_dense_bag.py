#!/usr/bin/env python3
"""One image of MakeBagDense on one MI355X: the per-box path (ife_bag_image given the explicit
dense box list) against the sliding-box-count path (ife_bag_image_dense), same process, warm runs.

  python scripts/bench_dense_bag.py [--size 96] [--box 15] [--bins 9] [--steps 5] [--warmup 1]
                                    [--out profiles/dense_bag.json]

Input: a synthetic float32 volume, the two-ellipsoid labels of synthetic.py, one scale, equalizing
edges of the foreground.  Both calls take host arrays and block, so a call is timed on the host
clock: upload, features, counting and the copy of the counts back are all inside, for both.  The
two count arrays must be equal.  Then the hipEvent time per kernel kind of one call of each
(IFE_OPT_PROFILE).  Writes the result to --out and prints it as one JSON line.

  python scripts/bench_dense_bag.py --stream [--out profiles/dense_stream.json]

times, at the same configuration and in one process, ife_bag_image_dense (the yardstick) against
the stream of row blocks (ife_bag_dense_stream_*) delivering frequencies: as one block, and with a
bound of an eighth of the bag; per-kind kernel times of each."""
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


def dense_boxes(gen, size):
    """DenseROIGenerator::generate in numpy: centres in raster order whose box fits."""
    sx, sy, sz = size
    nz, ny, nx = gen.shape
    z, y, x = np.nonzero(gen)
    x0, y0, z0 = x - sx // 2, y - sy // 2, z - sz // 2
    ok = (x0 >= 0) & (y0 >= 0) & (z0 >= 0) & (x0 + sx <= nx) & (y0 + sy <= ny) & (z0 + sz <= nz)
    n = int(ok.sum())
    return np.stack([x0[ok], y0[ok], z0[ok], np.full(n, sx), np.full(n, sy), np.full(n, sz)], 1).astype(np.int64)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def kernel_ms(pkg, ctx, fn):
    ctx.set_option(pkg.OPT_PROFILE, 1)
    ctx.reset_kernel_times()
    fn()
    kt = ctx.kernel_times()
    ctx.set_option(pkg.OPT_PROFILE, 0)
    return {k: {"launches": c, "total_ms": round(t, 4)} for k, (c, t) in kt.items()}


def spread(times):
    return {"median": round(statistics.median(times), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def stream_mode(args, pkg, ctx, img, lab, sigmas, size, edges, dense):
    """ife_bag_image_dense (the yardstick: the whole bag as counts in one host array) against the
    stream of row blocks delivering frequencies, each block dropped as the next arrives: one block
    (block_mb = 0) and a bound of an eighth of the bag."""
    counts, t_dense = timed(dense, args.steps, args.warmup)
    row_bytes = counts.shape[1] * counts.shape[2] * 4
    eighth_mb = max(1, round(len(counts) * row_bytes / 8 / 2 ** 20))
    s = counts.sum(-1, dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.float32(counts) / np.float32(s)[..., None]

    def stream(block_mb, keep=False):
        blocks = []
        for row0, rows in ctx.bag_image_dense_stream(img, lab, sigmas, size, edges, block_mb=block_mb):
            blocks.append((row0, rows) if keep else (row0, len(rows)))
        return blocks

    def phases(block_mb):
        """Host-clock milliseconds of _begin, of all _next calls and of _end of one warm stream."""
        import ctypes as C
        lib = pkg.load_library()
        d = pkg._desc(img.shape, (1.0, 1.0, 1.0))
        e32 = np.ascontiguousarray(edges, np.float32)
        n, cap, row0, got = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        t0 = time.perf_counter()
        rc = lib.ife_bag_dense_stream_begin(ctx._h, img.ctypes.data, pkg.F32, lab.ctypes.data, pkg._MSK_DT[lab.dtype],
                                            None, pkg.U8, C.byref(d), pkg._sigma_arg(sigmas), len(sigmas),
                                            pkg._size_arg(size), e32.ctypes.data, e32.shape[1], pkg.BAG_FREQUENCIES,
                                            block_mb, C.byref(n), C.byref(cap), pkg.MEM_HOST)
        t1 = time.perf_counter()
        rows = np.empty((max(cap.value, 1),) + counts.shape[1:], np.float32)
        rows[:] = 0                                   # touched: no page fault inside the copies
        t2 = time.perf_counter()
        while rc == 0:
            rc = lib.ife_bag_dense_stream_next(ctx._h, rows.ctypes.data, rows.shape[0], C.byref(row0), C.byref(got))
            if got.value == 0:
                break
        t3 = time.perf_counter()
        rc = rc or lib.ife_bag_dense_stream_end(ctx._h)
        t4 = time.perf_counter()
        if rc:
            sys.exit("stream call failed: %d" % rc)
        return {"begin": round((t1 - t0) * 1e3, 3), "next_all": round((t3 - t2) * 1e3, 3),
                "end": round((t4 - t3) * 1e3, 3)}

    runs, equal = {}, True
    for name, block_mb in (("stream_one_block", 0), ("stream_eighths", eighth_mb)):
        kept = stream(block_mb, keep=True)
        got = np.concatenate([rows for _, rows in kept])
        equal = equal and got.shape == want.shape and bool(
            np.array_equal(got[s != 0].view(np.uint32), want[s != 0].view(np.uint32)) and np.isnan(got[s == 0]).all())
        del kept, got
        blocks, times = timed(lambda: stream(block_mb), args.steps, args.warmup)
        runs[name] = {"block_mb": block_mb, "blocks": len(blocks), "largest_block_rows": max(n for _, n in blocks),
                      "ms": spread(times), "phases_ms": phases(block_mb),
                      "kernels": kernel_ms(pkg, ctx, lambda: stream(block_mb))}
    ms_dense = statistics.median(t_dense)
    out = {
        "metric": "one image of MakeBagDense: ife_bag_image_dense (counts, whole bag) over the stream of row "
                  "blocks (frequencies, one block), host arrays in and out",
        "value": round(ms_dense / runs["stream_one_block"]["ms"]["median"], 2), "unit": "x",
        "higher_is_better": True, "n_gpus": 1,
        "shape": list(img.shape), "box": list(size), "bins": args.bins, "sigmas": sigmas,
        "regions": int(len(counts)), "bag_bytes": int(len(counts) * row_bytes),
        "steps": args.steps, "warmup": args.warmup, "data": "synthetic (two ellipsoids, unit spacing)",
        "dense_ms": spread(t_dense), "dense_kernels": kernel_ms(pkg, ctx, dense),
        "frequencies_equal": equal,
    }
    out.update(runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not equal:
        sys.exit("the streamed frequencies differ from those of the dense counts")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--box", type=int, default=15)
    ap.add_argument("--bins", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stream", action="store_true",
                    help="time ife_bag_image_dense against the stream of row blocks (one block, about eight)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "dense_stream.json" if args.stream else "dense_bag.json")
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synthetic")
    ctx = pkg.Context(0)   # raises when there is no gfx950 device: no number without a GPU
    shape, size, sigmas = (args.size,) * 3, (args.box,) * 3, [1.0]
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    lab = synth.mask_ellipsoids(shape)
    clamped = np.minimum(lab, 1).astype(np.uint8)
    # histogram specification: equalizing edges of the foreground at this scale
    feat = ctx.emphysema_features(img, clamped, sigmas)[0]
    edges = np.stack([ctx.equalized_edges(ctx.sort_f32(feat[..., c][clamped != 0]), args.bins) for c in range(8)])
    boxes = dense_boxes(lab, size)

    def per_box():
        return ctx.bag_image(img, lab, sigmas, boxes, edges)

    def dense():
        return ctx.bag_image_dense(img, lab, sigmas, size, edges)

    if args.stream:
        return stream_mode(args, pkg, ctx, img, lab, sigmas, size, edges, dense)
    want, t_box = timed(per_box, args.steps, args.warmup)
    got, t_dense = timed(dense, args.steps, args.warmup)
    equal = bool(got.shape == want.shape and np.array_equal(got, want))
    ms_box, ms_dense = statistics.median(t_box), statistics.median(t_dense)
    out = {
        "metric": "one image of MakeBagDense: per-box counting over sliding box counts, host arrays in and out",
        "value": round(ms_box / ms_dense, 2), "unit": "x", "higher_is_better": True, "n_gpus": 1,
        "shape": list(shape), "box": list(size), "bins": args.bins, "sigmas": sigmas,
        "regions": int(len(boxes)), "foreground_fraction": round(float(clamped.mean()), 4),
        "steps": args.steps, "warmup": args.warmup, "data": "synthetic (two ellipsoids, unit spacing)",
        "per_box_ms": {"median": round(ms_box, 3), "min": round(min(t_box), 3), "max": round(max(t_box), 3)},
        "dense_ms": {"median": round(ms_dense, 3), "min": round(min(t_dense), 3), "max": round(max(t_dense), 3)},
        "counts_equal": equal,
        "per_box_kernels": kernel_ms(pkg, ctx, per_box),
        "dense_kernels": kernel_ms(pkg, ctx, dense),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not equal:
        sys.exit("the dense counts differ from the per-box counts")


if __name__ == "__main__":
    main()
