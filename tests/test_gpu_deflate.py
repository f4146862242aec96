"""ife_deflate on the device against the Python restatement of its block format
(tests/deflate_oracle.py): the device bytes equal the restatement's bytes, they inflate to the
input through zlib, and the CRC is zlib's.  Then the deflated fetch of the scale stream and the
tool that writes .nii.gz through it."""
import gzip
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_oracle as dfo  # noqa: E402
import niftiio  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "image-feature-extraction_amd", "host")
BIN = os.path.join(HOST, "bin")
C = dfo.C


@pytest.fixture(scope="module")
def cases():
    """name -> (input bytes, the restatement's blocks), computed once."""
    return {k: (v, dfo.deflate_blocks(v)) for k, v in dfo.small_cases().items()}


def check(ctx, data, want):
    got, crc = ctx.deflate(np.frombuffer(data, np.uint8))
    assert len(got) == len(want), (len(got), len(want))
    assert got == want
    assert dfo.inflate(got) == data
    assert crc == zlib.crc32(data)


@pytest.mark.parametrize("n", dfo.SIZES)
def test_sizes_zero_and_random(ctx, cases, n):
    check(ctx, *cases["zeros_%d" % n])
    data, want = cases["random_%d" % n]
    assert len(want) == n + 5 * ((n + C - 1) // C)  # random bytes come out stored
    check(ctx, data, want)


def test_constant_floats(ctx, cases):
    check(ctx, *cases["ones_f32"])


@pytest.mark.parametrize("L", dfo.RUN_LENGTHS)
def test_planted_runs(ctx, cases, L):
    for at in dfo.run_offsets(L):
        data, want = cases["run_%d_at_%d" % (L, at)]
        assert want[0] != 0  # chunk 0 took form F
        check(ctx, data, want)


def test_masked_volume(ctx, cases):
    check(ctx, *cases["masked_volume"])


def test_runs_that_cross_chunk_starts(ctx, cases):
    check(ctx, *cases["crossing_runs"])


def device_call(ife, ctx, data, src_off, dst_off, capacity=None):
    """ife_deflate over device pointers src + src_off -> dst + dst_off with 0xA5 guards around the
    output; returns (blocks or None, crc, needed, guards untouched)."""
    import torch
    n = len(data)
    cap = ctx.deflate_bound(n) if capacity is None else capacity
    assert 0 <= src_off < 16 and 0 <= dst_off < 16
    src = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    src[src_off:src_off + n] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dst = torch.full((cap + 64 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    # the offsets are the misalignments only from 16-byte aligned allocations
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    at = 32 + dst_off
    try:
        nout, crc = ctx.deflate_device(src.data_ptr() + src_off, n, dst.data_ptr() + at, cap)
    except ife.IfeError as e:
        assert e.code == ife.E_SIZE
        host = dst.cpu().numpy()
        return None, None, e.needed, bool((host == 0xA5).all())
    host = dst.cpu().numpy()
    clean = bool((host[:at] == 0xA5).all() and (host[at + nout:] == 0xA5).all())
    return host[at:at + nout].tobytes(), crc, nout, clean


@pytest.mark.parametrize("src_off", (1, 2, 3))
@pytest.mark.parametrize("dst_off", (1, 2, 3))
def test_misaligned_device_pointers(ife, ctx, cases, src_off, dst_off):
    for name in ("masked_volume", "random_%d" % (2 * C + 7), "run_259_at_%d" % (C - 1)):
        data, want = cases[name]
        got, crc, nout, clean = device_call(ife, ctx, data, src_off, dst_off)
        assert got == want and clean, name
        assert dfo.inflate(got) == data and crc == zlib.crc32(data)


def test_capacity_one_byte_short(ife, ctx, cases):
    for name in ("masked_volume", "random_%d" % (C + 1)):
        data, want = cases[name]
        got, _, needed, clean = device_call(ife, ctx, data, 0, 0, capacity=len(want) - 1)
        assert got is None and needed == len(want) and clean, name
        got, _, nout, clean = device_call(ife, ctx, data, 0, 0, capacity=len(want))
        assert got == want and nout == len(want) and clean, name


@pytest.mark.parametrize("src_off", range(16))
def test_every_source_alignment(ife, ctx, cases, src_off):
    """Every misalignment of the source against its 16-byte granules (the four word shifts of the
    load times the four byte shifts), and a source that ends with thread 0's eighth granule or
    one byte into its ninth."""
    dst_off = (5 * src_off + 3) % 16
    names = ["masked_volume", "random_%d" % (2 * C + 7), "run_259_at_%d" % (C - 1)]
    names += ["edge_%d" % n for n in dfo.edge_counts(src_off)]
    for name in names:
        data, want = cases[name]
        got, crc, nout, clean = device_call(ife, ctx, data, src_off, dst_off)
        assert got == want and clean, name
        assert dfo.inflate(got) == data and crc == zlib.crc32(data), name


@pytest.mark.parametrize("dst_off", range(16))
def test_every_destination_alignment_of_the_first_chunk(ife, ctx, cases, dst_off):
    """Chunk 0 at every alignment of the destination, in form F and in form S (from 12 on the
    stored header straddles a 16-byte slot); nothing is written outside the blocks."""
    for name in ("masked_volume", "random_%d" % (C + 1), "tie_1000_3"):
        data, want = cases[name]
        got, crc, nout, clean = device_call(ife, ctx, data, 0, dst_off)
        assert got == want and nout == len(want), name
        assert clean, name
        assert dfo.inflate(got) == data and crc == zlib.crc32(data), name


def test_form_tie_takes_stored(ife, ctx, cases):
    """Form F one byte longer than S, as long as S (the tie: stored) and one byte shorter; the
    size pass and the emit pass take the same form."""
    names = list(dfo.tie_cases())
    assert len(names) == 7
    for name in names:
        data, want = cases[name]
        n0, run = min(len(data), C), int(name.rsplit("_", 1)[1])
        behind = len(data) - n0  # the bytes of a second chunk come out stored
        assert len(want) == (n0 + 4 if run == 4 else n0 + 5) + (behind + 5 if behind else 0), name
        got, crc = ctx.deflate(np.frombuffer(data, np.uint8))
        assert len(got) == len(want), (name, len(got), len(want))
        assert (got[0] != 0) if run == 4 else (got[0] == 0), name
        assert got == want, name
        assert dfo.inflate(got) == data and crc == zlib.crc32(data), name
        got, _, needed, clean = device_call(ife, ctx, data, 0, 0, capacity=len(want) - 1)
        assert got is None and needed == len(want) and clean, name
        got, _, nout, clean = device_call(ife, ctx, data, 0, 0, capacity=len(want))
        assert got == want and nout == len(want) and clean, name


@pytest.mark.parametrize("L", dfo.SEAM_LENGTHS)
def test_runs_at_thread_and_wave_seams(ctx, cases, L):
    """Runs that begin and runs that end one byte before, at and one byte behind a thread's first
    byte, at least one of each at a wave's: the start and the end of a run as the scans hand them on."""
    data, want = cases["seams_%d" % L]
    assert want[0] != 0  # chunk 0 took form F
    check(ctx, data, want)


def test_null_pointers(ife, ctx):
    import ctypes as Ct
    n, crc = Ct.c_size_t(), Ct.c_uint32()
    buf = np.zeros(64, np.uint8)
    lib, h, p = ife.load_library(), ctx._h, buf.ctypes.data
    assert lib.ife_deflate(h, None, 8, p, 64, Ct.byref(n), Ct.byref(crc), ife.MEM_HOST) == ife.E_ARG
    assert lib.ife_deflate(h, p, 8, None, 64, Ct.byref(n), Ct.byref(crc), ife.MEM_HOST) == ife.E_ARG
    assert lib.ife_deflate(h, p, 8, p, 64, None, Ct.byref(crc), ife.MEM_HOST) == ife.E_ARG
    assert lib.ife_deflate(h, p, 8, p, 64, Ct.byref(n), None, ife.MEM_HOST) == ife.E_ARG


def test_more_chunks_than_a_scan_tile(ctx):
    """4097 chunks and 5 bytes of masked random floats: the second tile of the offset scan and a
    short last chunk.  Inflate and CRC only."""
    n = 4097 * C + 5
    rng = np.random.default_rng(17)
    v = rng.random((n + 3) // 4, dtype=np.float32)
    v[(np.arange(v.size) // 1500) % 6 != 0] = 0  # about 16 % foreground
    data = v.view(np.uint8)[:n].tobytes()
    got, crc = ctx.deflate(np.frombuffer(data, np.uint8))
    assert len(got) <= dfo.bound(n) and len(got) < n // 3
    assert crc == zlib.crc32(data)
    assert dfo.inflate(got) == data


def stream_planes_deflated(ife, ctx, synth, shape):
    """Every plane of a planar two-scale stream fetched deflated: it inflates to the plane that
    fetch returns and has its CRC.  Returns the largest block size."""
    img = synth.volume_f32(shape, 7)
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    largest = 0
    with ctx.scale_stream(img, mask, [1.0, 2.0], layout=ife.PLANAR) as st:
        for scale in (1, 0):
            planes = st.fetch(scale)
            assert planes.shape == (8,) + shape
            for comp in range(8):
                blocks, crc = st.fetch_deflated(scale, comp)
                raw = planes[comp].tobytes()
                assert dfo.inflate(blocks) == raw, (shape, scale, comp)
                assert blocks == dfo.deflate_blocks(raw), (shape, scale, comp)
                assert crc == zlib.crc32(raw)
                assert len(blocks) < len(raw)
                largest = max(largest, len(blocks))
    return largest


@pytest.mark.parametrize("differential", (0, 1))
def test_stream_fetch_deflated_of_planes_off_the_granule(ife, synth, differential):
    """Planes whose size is no multiple of 16 bytes lie 0, 12, 8 and 4 (then 0, 4, 8 and 12) bytes
    behind a 16-byte boundary; the larger planes behind the smaller ones, on one fresh context,
    take more than the block buffer holds by then, so it has to grow."""
    small, large = (9, 11, 13), (21, 25, 41)
    with ife.Context(0) as c:
        c.set_option(ife.OPT_DIFFERENTIAL, differential)
        for shape, nchunks in ((small, 1), (large, 3)):
            plane = 4 * shape[0] * shape[1] * shape[2]
            assert plane % 16 != 0 and (plane + C - 1) // C == nchunks
            # a stream's planes follow each other from a 16-byte aligned allocation
            assert sorted({(comp * plane) % 16 for comp in range(8)}) == [0, 4, 8, 12]
            largest = stream_planes_deflated(ife, c, synth, shape)
            if shape == small:  # the buffer holds no more than this after the small planes
                held = dfo.bound(plane)
        assert largest > held


@pytest.mark.parametrize("differential", (0, 1))
def test_stream_fetch_deflated(ife, ctx, synth, differential):
    shape = (20, 24, 40)
    img = synth.volume_f32(shape, 7)
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    ctx.set_option(ife.OPT_DIFFERENTIAL, differential)
    try:
        with ctx.scale_stream(img, mask, [1.0, 2.0], layout=ife.PLANAR) as st:
            for scale in (1, 0):
                planes = st.fetch(scale)
                assert planes.shape == (8,) + shape
                for comp in range(8):
                    blocks, crc = st.fetch_deflated(scale, comp)
                    raw = planes[comp].tobytes()
                    assert dfo.inflate(blocks) == raw, (scale, comp)
                    assert crc == zlib.crc32(raw)
                    assert len(blocks) < len(raw)
        with ctx.scale_stream(img, mask, [1.0], layout=ife.INTERLEAVED) as st:
            with pytest.raises(ife.IfeError) as e:
                st.fetch_deflated(0, 0)
            assert e.value.code == ife.E_STATE
            assert st.fetch(0).shape == shape + (8,)
    finally:
        ctx.set_option(ife.OPT_DIFFERENTIAL, 0)


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "image-feature-extraction_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return BIN


def run_extract(tmp_path, out, **env_add):
    env = dict(os.environ)
    for k in ("IFE_DEVICES", "IFE_DEVICE_GZIP", "IFE_OUT_FILE_TYPE"):
        env.pop(k, None)
    env.update(env_add)
    (tmp_path / out).mkdir()
    return subprocess.run([os.path.join(BIN, "ExtractFeatures"), "-i", str(tmp_path / "i.nii.gz"), "-m",
                           str(tmp_path / "m.nii.gz"), "-o", str(tmp_path / out / "o"), "-s", "1", "-s", "2.5"],
                          capture_output=True, text=True, env=env)


# planes of a multiple of 16 bytes, and of 12 bytes more than one
@pytest.mark.parametrize("shape", ((24, 28, 32), (13, 15, 17)), ids=("24x28x32", "13x15x17"))
def test_extract_features_device_gzip(built, tmp_path, synth, shape):
    niftiio.write(str(tmp_path / "i.nii.gz"), synth.volume_f32(shape, 5), (0.9, 1.0, 1.1))
    niftiio.write(str(tmp_path / "m.nii.gz"), np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8),
                  (0.9, 1.0, 1.1))
    r = run_extract(tmp_path, "host")
    assert r.returncode == 0, r.stderr
    r = run_extract(tmp_path, "device", IFE_DEVICE_GZIP="1")
    assert r.returncode == 0, r.stderr
    names = sorted(os.listdir(tmp_path / "host"))
    assert len(names) == 16 and names == sorted(os.listdir(tmp_path / "device"))
    for f in names:
        a = gzip.decompress((tmp_path / "host" / f).read_bytes())   # checks CRC and length
        b = gzip.decompress((tmp_path / "device" / f).read_bytes())
        assert len(a) == 352 + 4 * shape[0] * shape[1] * shape[2] and a == b, f
    # one device only
    r = run_extract(tmp_path, "both", IFE_DEVICE_GZIP="1", IFE_DEVICES="0,0")
    assert r.returncode != 0 and "IFE_DEVICES" in r.stderr
