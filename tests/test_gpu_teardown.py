"""Device memory comes back: what a context, a Samples object, a dense stream or a Multi allocated
is free again after its teardown.

Every case runs ordinary calls on host (numpy) inputs, so that nothing but the library allocates
between the two readings of torch.cuda.mem_get_info(), and runs once beforehand in a throw-away
context: the runtime's own lazy allocations (code objects, scratch, copy streams) then lie before
the first reading.

Volume 128 x 128 x 64, one float field of it 4 MiB.  The loss must stay below one field: that is
less than every volume-sized buffer a context can hold, so a single one left behind fails.  The
bound follows from the shape, it is not measured.  Losses measured on an MI355X, the same before
and after the buffers became owners of their allocations: 0 bytes in every case but the ended
dense stream, 2 MiB there (the stream's copy stream is created at the first _begin and lives on
with the context).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (64, 128, 128)                      # z, y, x
FIELD = 4 * SHAPE[0] * SHAPE[1] * SHAPE[2]  # bytes of one float field
SIGMAS = [1.5]
SIZE = (5, 5, 5)
N_EDGES = 8
STREAM_SCRATCH_MB = 64  # the stream's blocks get an eighth of what features and codes leave: < 3 MiB


@pytest.fixture(scope="module")
def vol():
    rng = np.random.default_rng(20)
    img = rng.standard_normal(SHAPE, np.float32) * 100 - 500
    lab = np.zeros(SHAPE, np.uint8)
    lab[8:-8, 8:-8, 8:-8] = 1               # a solid interior
    gen = np.zeros(SHAPE, np.uint8)
    gen[16:48, 32:96, 32:96] = 1            # 32 centre planes of 4096 regions, 36 MiB of rows
    edges = np.tile(np.linspace(-600, 400, N_EDGES, dtype=np.float32), (8 * len(SIGMAS), 1))
    rois = np.array([[10, 10, 10, 20, 20, 20], [40, 50, 20, 31, 17, 9]], np.int64)
    return dict(img=img, lab=lab, gen=gen, edges=edges, rois=rois)


def free_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


def loss_across_context(ife, sequence):
    """Free memory before a context exists minus free memory after its destruction, with
    sequence(ctx) in between; the whole once before in a throw-away context."""
    free_bytes()
    with ife.Context(0) as warm:
        sequence(warm)
    before = free_bytes()
    ctx = ife.Context(0)
    try:
        sequence(ctx)
    finally:
        ctx.close()
    return before - free_bytes()


def loss_on_live_context(ife, prepare, sequence):
    """Free memory before sequence(ctx) minus after, the context alive at both readings and
    prepare(ctx) done before the first (what it allocates is the context's to keep)."""
    free_bytes()
    with ife.Context(0) as warm:
        prepare(warm)
        sequence(warm)
    with ife.Context(0) as ctx:
        prepare(ctx)
        before = free_bytes()
        sequence(ctx)
        return before - free_bytes()


def check(name, loss):
    print("%s: %d bytes lost (bound %d)" % (name, loss, FIELD))
    assert loss < FIELD


def stream_begin(ctx, ife, vol):
    """ife_bag_dense_stream_begin with a budget that makes many blocks; (regions, rows of the largest block)."""
    lib = ife.load_library()
    ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, STREAM_SCRATCH_MB)
    d = ife._desc(SHAPE, (1.0, 1.0, 1.0))
    n, cap = C.c_int64(-1), C.c_int64(-1)
    rc = lib.ife_bag_dense_stream_begin(ctx._h, vol["img"].ctypes.data, ife.F32, vol["lab"].ctypes.data, ife.U8,
                                        vol["gen"].ctypes.data, ife.U8, C.byref(d), ife._sigma_arg(SIGMAS),
                                        len(SIGMAS), (C.c_int64 * 3)(*SIZE), vol["edges"].ctypes.data, N_EDGES,
                                        ife.BAG_COUNTS, 0, C.byref(n), C.byref(cap), ife.MEM_HOST)
    assert rc == ife.OK, lib.ife_last_error(ctx._h)
    assert n.value == int(vol["gen"].sum()) and n.value > 2 * cap.value  # at least three blocks
    return n.value, cap.value


def stream_first_block(ctx, ife, vol):
    lib = ife.load_library()
    _, cap = stream_begin(ctx, ife, vol)
    rows = np.empty((cap, 8 * len(SIGMAS), N_EDGES + 1), np.uint32)
    row0, got = C.c_int64(-1), C.c_int64(-1)
    rc = lib.ife_bag_dense_stream_next(ctx._h, rows.ctypes.data, cap, C.byref(row0), C.byref(got))
    assert rc == ife.OK, lib.ife_last_error(ctx._h)
    assert row0.value == 0 and 0 < got.value <= cap


def test_every_family_on_one_context(ife, vol):
    def sequence(ctx):
        feats = ctx.emphysema_features(vol["img"], vol["lab"], SIGMAS)
        ctx.normalized_gaussian_convolution(vol["img"], vol["lab"].astype(np.float32), SIGMAS[0])
        ctx.differential_features(vol["img"], vol["lab"], SIGMAS)
        ctx.signed_distance_map(vol["lab"])
        ctx.bag_image(vol["img"], vol["lab"], SIGMAS, vol["rois"], vol["edges"])
        bag = ctx.bag_image_dense(vol["img"], vol["lab"], SIGMAS, SIZE, vol["edges"], gen_mask=vol["gen"])
        rows = ctx.dense_roi_histograms(feats[0], vol["lab"], SIZE, vol["edges"], gen_mask=vol["gen"])
        assert len(bag) == len(rows) == int(vol["gen"].sum())

    check("every family, then destroy", loss_across_context(ife, sequence))


def test_streaming_call_left_unfinished(ife, vol):
    def sequence(ctx):
        lib = ife.load_library()
        d = ife._desc(SHAPE, (1.0, 1.0, 1.0))
        rc = lib.ife_emphysema_features_begin(ctx._h, vol["img"].ctypes.data, ife.F32, vol["lab"].ctypes.data,
                                              ife.U8, C.byref(d), ife._sigma_arg(SIGMAS), len(SIGMAS),
                                              ife.INTERLEAVED)
        assert rc == ife.OK, lib.ife_last_error(ctx._h)

    check("emphysema_features_begin without _end, then destroy", loss_across_context(ife, sequence))


def test_dense_stream_left_open_after_its_first_block(ife, vol):
    check("dense stream open after one block, then destroy",
          loss_across_context(ife, lambda ctx: stream_first_block(ctx, ife, vol)))


def test_dense_stream_end_releases_the_streams_own(ife, vol):
    def prepare(ctx):  # the staging buffers the stream shares with the whole-bag call
        ctx.set_option(ife.OPT_DENSE_SCRATCH_MB, STREAM_SCRATCH_MB)
        ctx.bag_image_dense(vol["img"], vol["lab"], SIGMAS, SIZE, vol["edges"], gen_mask=vol["gen"])

    def sequence(ctx):
        stream_first_block(ctx, ife, vol)
        assert ife.load_library().ife_bag_dense_stream_end(ctx._h) == ife.OK

    check("dense stream ended after one block, context alive", loss_on_live_context(ife, prepare, sequence))


def test_samples_object(ife, vol):
    picked = np.flatnonzero(vol["lab"])[::7][None, :]

    def sequence(ctx):
        s = ctx.samples(8 * len(SIGMAS))
        s.add_image(vol["img"], vol["lab"], SIGMAS)                      # fused branch, first capacity
        s.add_image(vol["img"], vol["lab"], SIGMAS, indices=picked)      # sampled branch, capacity doubles
        s.add_image(vol["img"], vol["lab"], SIGMAS)                      # and doubles again
        assert s.count() == 2 * int(vol["lab"].sum()) + picked.size
        s.sort()
        s.equalized_edges(N_EDGES + 1)
        s.close()

    # once before on the same context: what the context itself keeps is there at the first reading
    check("samples object closed, context alive", loss_on_live_context(ife, sequence, sequence))


def test_multi_with_the_device_twice(ife, vol):
    def sequence():
        m = ife.Multi([0, 0])
        try:
            m.emphysema_features(vol["img"], vol["lab"], SIGMAS)
        finally:
            m.close()

    free_bytes()
    sequence()
    before = free_bytes()
    sequence()
    check("Multi over the device twice, then close", before - free_bytes())
