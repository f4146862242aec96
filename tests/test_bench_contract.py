"""bench.py's output contract (one JSON line; the keys and meanings the driver reads), on a
small volume so that it takes seconds.  GPU only: the bench has no CPU path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout                       # exactly one line on stdout
    return json.loads(lines[0])


def assert_value_is_the_step_time(d, voxels_times_scales):
    """value and ms_per_step are one measurement, printed to 1 and 3 decimals: they agree to within
    those two roundings.  (Half a unit of the third decimal of a 0.4 ms step is 1.2e-3 of it, so a
    fixed relative 1e-3 failed now and then on this small volume.)"""
    from_ms = voxels_times_scales / (d["ms_per_step"] * 1e-3) / 1e6
    assert abs(d["value"] - from_ms) <= from_ms * 0.00051 / d["ms_per_step"] + 0.051, (d["value"], d["ms_per_step"])


def test_single_gpu_line():
    """--full: the headline plus everything measured beside it."""
    d = run_bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "64", "96", "128",
                  "--cpu-sample", "48", "--full")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"].startswith("Mvoxels/sec Hessian+eig") and d["unit"] == "Mvoxels/s"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert_value_is_the_step_time(d, 64 * 96 * 128 * 3)
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None and r["issue"] is None         # PMC figures exist only for the default workload
    assert r["measured_fill_GBs"] > 1000 and r["measured_copy_GBs"] > 1000   # the box's own stream rates
    assert r["kernels"]["features"]["alg_bytes_per_voxel"] == 37.0 and r["kernels"]["iir_y"]["alg_bytes_per_voxel"] == 6.0
    assert set(r["kernels"]) >= {"iir_z", "iir_x", "iir_y", "features", "prep"}
    assert r["kernels"]["features"]["launches_per_step"] == 3.0
    assert r["kernels"]["iir_z"]["launches_per_step"] == 1.0   # all (scale, field) jobs in one launch
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c


def test_slab_engine_line_with_one_rank():
    """The multi-GPU engine (one rank: no neighbour, so no transfer) prints the same contract,
    and its description comes from what the runner built."""
    d = run_bench("--gpus", "1", "--steps", "1", "--warmup", "1", "--size", "64", "64", "64",
                  "--force-slab", "--no-cpu-baseline", "--i16", "--spacing", "0.7", "0.7", "1.0", "--full")
    assert d["n_gpus"] == 1 and d["value"] > 0
    w = d["config"]["workload"]
    assert "1 Z-slabs" in w and "int16" in w and "spacing [0.7, 0.7, 1.0]" in w
    assert set(d["roofline"]["kernels"]) >= {"zslab_sweep", "zslab_combine", "iir_x", "iir_y", "features"}
    assert d["roofline"]["issue"] is None                      # PMC instruction counts exist only for the default workload
    assert "cpu_baseline" not in d


def test_per_rank_timing_proxy_is_marked_as_such():
    """--proxy-world: one GPU runs the local work of a rank with neighbours (no transfers);
    the line must say that it is no headline."""
    d = run_bench("--gpus", "1", "--steps", "1", "--warmup", "1", "--size", "64", "64", "64",
                  "--proxy-world", "4", "--proxy-rank", "1", "--no-cpu-baseline", "--full")
    assert d["headline"] is False and "rank 1 of 4" in d["config"]["proxy"]
    assert "4 Z-slabs" in d["config"]["workload"] and d["n_gpus"] == 1
    assert set(d["roofline"]["kernels"]) >= {"zslab_sweep", "zslab_combine", "iir_x", "iir_y", "features"}


def test_plain_line_is_the_headline_only():
    """Without --full the run sets up, warms up, times --steps steps and prints the line: no CPU
    baseline, no stream probe, no shortcut step, no oracle comparison."""
    d = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "64", "96", "128")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in d, k
    assert d["metric"].startswith("Mvoxels/sec Hessian+eig") and d["unit"] == "Mvoxels/s"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert_value_is_the_step_time(d, 64 * 96 * 128 * 3)
    assert "cpu_baseline" not in d and d["ms_per_step_with_constant_line_shortcut"] is None
    assert d["roofline"]["measured_fill_GBs"] is None and d["roofline"]["measured_copy_GBs"] is None
    assert d["roofline"]["kernels"]["features"]["launches_per_step"] == 3.0   # the timed steps' own events


def load_dump(tmp_path, name, *args):
    out = tmp_path / name
    run_bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out), *args)
    assert [p.name for p in out.iterdir()] == ["features.npy"]
    return np.load(out / "features.npy")


def test_dump_outputs_is_what_the_step_computed(tmp_path, synth, oracle):
    """A volume whose output fits the budget is written whole, [scale, voxel, feature], and is
    the filter's output: the bit-exact components equal the oracle, the eigen features within
    the double mode's bar."""
    from oracle.parity import assert_eig_parity
    shape = (24, 20, 28)
    got = load_dump(tmp_path, "whole", "--size", *map(str, shape), "--sigmas", "1", "2", "--trig", "0")
    assert got.dtype == np.float32 and got.shape == (2, 24 * 20 * 28, 8)
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    ones = np.ones(shape, np.uint8)
    for s, sigma in enumerate((1.0, 2.0)):
        ref = oracle.emphysema_features(img, ones, sigma)
        g = got[s].reshape(shape + (8,))
        assert np.array_equal(g[..., :2], ref[..., :2]), "sigma %g" % sigma
        assert_eig_parity(g, ref, 1e-6, "sigma %g" % sigma)


def test_dump_outputs_sample_is_fixed_across_layouts_and_engines(tmp_path):
    """A larger output is sampled at seeded voxels: the same sample, in the same order, from the
    interleaved and the planar layout and from the slab engine (one rank)."""
    size = ("64", "96", "128")
    a = load_dump(tmp_path, "interleaved", "--size", *size)
    b = load_dump(tmp_path, "planar", "--size", *size, "--layout", "planar")
    c = load_dump(tmp_path, "slab", "--size", *size, "--force-slab")
    assert a.dtype == np.float32 and a.shape[0] == 3 and a.shape[2] == 8
    assert 0 < a.nbytes <= 64 << 20 and a.shape[1] < 64 * 96 * 128
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a, b) and np.array_equal(a, c)
