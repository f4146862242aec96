"""The shared causal sweep of the first axis pass (IFE_OPT_Z_SWEEP): one launch reads image and
mask, leaves the two float sources and the checkpoints of every scale of a group, and the line
kernel proper then sweeps backward only.  It must give the bits of the path it replaces (the
prepass and one full line kernel per job, option off), which is run in the same test.

Z lengths sit on and around one register block and one, two and three pairs of the default
block (12): a line of one pair gets sources only, a last pair of one sample, exact multiples,
the first length with a checkpointed pair, and two lengths long enough for the steady loops of
both launches.  Line counts (ny * nx) are no multiples of 64 or 256.  Every comparison between
two device paths is on uint32 views.

The emphysema entry points take uint8 and uint16 masks only (a float mask is IFE_E_ARG before
any kernel runs), so the weighted case is a uint16 mask whose values 0, 1, 2, 3, 7 are the
certainty: weights other than one, and exact zeros.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Z_LENGTHS = [4, 5, 23, 24, 25, 47, 48, 49, 72, 73, 100, 160]
# 63, 65, 130, 300, 279 lines; 621 lines with nx % 4 == 3.  (Two waves and a line or two: 5 x 26,
# since the entry point refuses an axis shorter than four voxels and 129 = 3 x 43 has no other form.)
PLANES = [(7, 9), (5, 13), (5, 26), (4, 75), (9, 31), (23, 27)]
CASES = [([1.0, 2.5, 4.0], (1.0, 1.0, 1.0)), ([4.0, 1.0, 2.5], (0.7, 0.8, 1.25))]
FIVE = [1.0, 2.5, 4.0, 2.5, 1.0]

_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(synth, shape, kind="f32_u8"):
    """(image, mask) of one of the input kinds, made once per shape and read-only."""
    key = (shape, kind)
    if key not in _cache:
        labels = synth.mask_ellipsoids(shape)
        labels[0, 0, 0] = 1
        img = synth.volume_i16(shape, 77) if kind.startswith("i16") else synth.volume_f32(shape, 1234)
        if kind.endswith("_u8"):
            mask = np.minimum(labels, 1).astype(np.uint8)
        elif kind.endswith("_u16w"):
            w = np.array([1, 2, 3, 7], np.uint16)[np.arange(labels.size).reshape(shape) % 4]
            mask = np.where(labels > 0, w, 0).astype(np.uint16)
            assert (mask == 0).any() and (mask > 1).any()
        else:
            mask = None
        img.setflags(write=False)
        if mask is not None:
            mask.setflags(write=False)
        _cache[key] = (img, mask)
    return _cache[key]


class _Options:
    def __init__(self, ctx, ife, **opts):
        self.ctx, self.ife, self.opts = ctx, ife, opts
        self.defaults = {"OPT_Z_SWEEP": 1, "OPT_CONST_LINES": 1, "OPT_IIR_BLOCK": 0, "OPT_IIR_CKPT": 2,
                         "OPT_IIR_FMA": 0}

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(getattr(self.ife, k), v)

    def __exit__(self, *a):
        for k in self.opts:
            self.ctx.set_option(getattr(self.ife, k), self.defaults[k])


def _run(ctx, ife, img, mask, sigmas, spacing=(1.0, 1.0, 1.0), **opts):
    with _Options(ctx, ife, **opts):
        return ctx.emphysema_features(img, mask, sigmas, spacing)


def _on_equals_off(ctx, ife, img, mask, sigmas, spacing=(1.0, 1.0, 1.0), **opts):
    """Runs both paths with the same further options; returns the sweep's result."""
    keep = (img.copy(), None if mask is None else mask.copy())
    on = _run(ctx, ife, img, mask, sigmas, spacing, OPT_Z_SWEEP=1, **opts)
    off = _run(ctx, ife, img, mask, sigmas, spacing, OPT_Z_SWEEP=0, **opts)
    assert on.shape == (len(sigmas),) + img.shape + (8,)
    for s in range(len(sigmas)):
        assert np.array_equal(_bits(on[s]), _bits(off[s])), "scale %d of %s" % (s, sigmas)
    assert np.array_equal(img, keep[0]) and (mask is None or np.array_equal(mask, keep[1]))
    return on


@pytest.mark.parametrize("sigmas,spacing", CASES)
@pytest.mark.parametrize("i,nz", list(enumerate(Z_LENGTHS)))
def test_sweep_equals_prepass_path_at_every_cut(ctx, ife, synth, i, nz, sigmas, spacing):
    ny, nx = PLANES[i % len(PLANES)]
    img, mask = _inputs(synth, (nz, ny, nx))
    _on_equals_off(ctx, ife, img, mask, sigmas, spacing)


@pytest.mark.parametrize("ny,nx", PLANES)
@pytest.mark.parametrize("nz", [25, 73])
def test_sweep_equals_prepass_path_at_every_line_count(ctx, ife, synth, nz, ny, nx):
    img, mask = _inputs(synth, (nz, ny, nx))
    _on_equals_off(ctx, ife, img, mask, [2.5, 1.0, 4.0], (0.7, 0.8, 1.25))


@pytest.mark.parametrize("ns", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("shape", [(49, 5, 13), (100, 9, 31)])
def test_one_to_five_scales(ctx, ife, synth, shape, ns):
    """Four and five scales run as two groups: the second finds the sources the first left."""
    img, mask = _inputs(synth, shape)
    _on_equals_off(ctx, ife, img, mask, FIVE[:ns], (0.7, 0.8, 1.25))


@pytest.mark.parametrize("kind", ["f32_u8", "i16_u8", "f32_u16w", "i16_u16w", "f32_none", "i16_none"])
@pytest.mark.parametrize("shape", [(24, 7, 9), (73, 4, 75)])
def test_input_types_against_option_off_and_oracle(ctx, ife, oracle, synth, shape, kind):
    """No mask and a float image: no source is written, the backward launch reads the image."""
    from test_gpu_parity import assert_features_close
    img, mask = _inputs(synth, shape, kind)
    sigmas = FIVE[:4]
    on = _on_equals_off(ctx, ife, img, mask, sigmas, (0.7, 0.8, 1.25))
    weights = np.ones(shape, np.uint8) if mask is None else mask
    for s in (0, 3):  # one scale of each group
        ref = oracle.emphysema_features(img.astype(np.float32), weights, sigmas[s], (0.7, 0.8, 1.25))
        assert_features_close(on[s], ref, mask)


@pytest.mark.parametrize("kind,idt,mdt", [("f32_u8", "F32", "U8"), ("i16_u16w", "I16", "U16"),
                                          ("f32_none", "F32", "U8"), ("i16_none", "I16", "U8")])
def test_device_pointers_aligned_to_the_element_only(ctx, ife, synth, kind, idt, mdt):
    """Image and mask one element into their allocations: nothing in the sweep needs more than
    element alignment.  Neither buffer is written."""
    import torch
    shape = (49, 9, 31)
    img, mask = _inputs(synth, shape, kind)
    n = img.size

    def dev(a):
        flat = np.concatenate([np.full(1, 3, a.dtype), a.ravel(), np.full(1, 5, a.dtype)])
        bytes_ = torch.from_numpy(flat.view(np.uint8).copy()).cuda()
        return bytes_, bytes_.data_ptr() + a.itemsize
    di, pi = dev(img)
    dm, pm = dev(mask) if mask is not None else (None, None)
    assert pi % 16 != 0
    want_i = di.cpu().numpy().copy()
    want_m = None if dm is None else dm.cpu().numpy().copy()
    sigmas = [1.0, 2.5, 4.0]
    res = {}
    for opt in (1, 0):
        out = torch.full((3, 8) + shape, 7.0, dtype=torch.float32, device="cuda")
        with _Options(ctx, ife, OPT_Z_SWEEP=opt):
            ctx.emphysema_features_device(pi, getattr(ife, idt), pm, getattr(ife, mdt), shape,
                                          (1.0, 1.0, 1.0), sigmas, out.data_ptr(), ife.PLANAR)
            ctx.synchronize()
        res[opt] = out.cpu().numpy()
    assert np.array_equal(_bits(res[1]), _bits(res[0]))
    host = ctx.emphysema_features(img, mask, sigmas, layout=ife.PLANAR)
    assert np.array_equal(_bits(res[1]), _bits(host)) and n == np.prod(shape)
    assert np.array_equal(di.cpu().numpy(), want_i)
    assert dm is None or np.array_equal(dm.cpu().numpy(), want_m)


def _const_volumes(synth, shape):
    nz, ny, nx = shape
    ones = (synth.volume_f32(shape, 5).copy(), np.ones(shape, np.uint8))  # every denominator line constant
    ct = synth.volume_i16(shape, 9).astype(np.int32)
    ct = (-(np.abs(ct) % 1000) - 1).astype(np.int16)          # negative everywhere: T * 0 is -0 outside
    cmask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    cmask[:, : ny // 2, :] = 0                                # whole Z lines of exterior
    tail = np.abs(synth.volume_f32(shape, 6)) + np.float32(1)  # T * 0 is +0 in front of the last samples
    tmask = np.zeros(shape, np.uint8)
    tmask[nz - 1, ::2, :] = 1                                 # only the last sample of every other row of lines
    tmask[nz - 5:, :, 1] = 1                                  # ... and the last five of one column
    return {"ones": ones, "ct": (ct, cmask), "tail": (tail, tmask)}


@pytest.mark.parametrize("name", ["ones", "ct", "tail"])
@pytest.mark.parametrize("shape", [(49, 9, 31), (100, 23, 27), (24, 7, 9)])
def test_constant_lines(ctx, ife, synth, shape, name):
    """The per-line record of the sweep against the registers of the full kernel: an all-ones
    mask, a CT-like volume whose exterior is -0 in the numerator and +0 in the denominator, and
    lines that are constant up to their last pair only."""
    img, mask = _const_volumes(synth, shape)[name]
    if name == "ct":
        assert (img < 0).all() and (mask[:, 0, 0] == 0).all()
    sigmas = [1.0, 2.5, 4.0]
    short = _on_equals_off(ctx, ife, img, mask, sigmas, OPT_CONST_LINES=1)
    plain = _on_equals_off(ctx, ife, img, mask, sigmas, OPT_CONST_LINES=0)
    assert np.array_equal(_bits(short), _bits(plain))


@pytest.mark.parametrize("block", [8, 10, 12, 16])
@pytest.mark.parametrize("shape", [(49, 5, 13), (100, 4, 75)])
def test_every_block_size(ctx, ife, synth, shape, block):
    img, mask = _inputs(synth, shape)
    got = _on_equals_off(ctx, ife, img, mask, [1.0, 2.5, 4.0], (0.7, 0.8, 1.25), OPT_IIR_BLOCK=block)
    assert np.array_equal(_bits(got), _bits(_run(ctx, ife, img, mask, [1.0, 2.5, 4.0], (0.7, 0.8, 1.25))))


@pytest.mark.parametrize("shape", [(49, 5, 13), (100, 4, 75)])
def test_block_checkpoints_keep_the_old_path(ctx, ife, synth, shape):
    """IFE_OPT_IIR_CKPT=1 runs the prepass and the per-block kernel whatever the sweep option
    says, and gives the same bits."""
    img, mask = _inputs(synth, shape)
    sigmas = [1.0, 2.5, 4.0]
    ctx.reset_kernel_times()
    with _Options(ctx, ife, OPT_IIR_CKPT=1):
        ctx.set_option(ife.OPT_PROFILE, 1)
        try:
            per_block = ctx.emphysema_features(img, mask, sigmas)
            ctx.synchronize()
            times = ctx.kernel_times()
        finally:
            ctx.set_option(ife.OPT_PROFILE, 0)
    assert times["prep"][0] == 1 and times["iir_z"][0] == 1
    assert np.array_equal(_bits(per_block), _bits(_run(ctx, ife, img, mask, sigmas)))


@pytest.mark.parametrize("shape", [(49, 5, 13), (100, 4, 75)])
def test_fused_build(ctx, ife, synth, shape):
    img, mask = _inputs(synth, shape)
    _on_equals_off(ctx, ife, img, mask, [1.0, 2.5, 4.0], (0.7, 0.8, 1.25), OPT_IIR_FMA=1)


@pytest.mark.parametrize("kind", ["f32_u8", "i16_none"])
def test_streaming_form_equals_one_call(ctx, ife, synth, kind):
    shape = (73, 9, 31)
    img, mask = _inputs(synth, shape, kind)
    sigmas = [1.0, 2.5, 4.0]
    whole = _run(ctx, ife, img, mask, sigmas, OPT_Z_SWEEP=0)
    vols = list(ctx.emphysema_features_stream(img, mask, sigmas))
    assert len(vols) == 3
    for k, vol in enumerate(vols):
        assert np.array_equal(_bits(vol), _bits(whole[k]))


def test_workspace_grows_and_shrinks(ife, synth):
    """A fresh context: small, then larger (every workspace is reallocated), then small again."""
    small, large = (25, 5, 13), (100, 23, 27)
    sigmas = [1.0, 2.5, 4.0]
    with ife.Context(0) as off:
        off.set_option(ife.OPT_TRIG_MODE, 0)
        off.set_option(ife.OPT_Z_SWEEP, 0)
        want = {s: off.emphysema_features(*_inputs(synth, s), sigmas) for s in (small, large)}
    with ife.Context(0) as c:
        c.set_option(ife.OPT_TRIG_MODE, 0)
        for shape in (small, large, small):
            got = c.emphysema_features(*_inputs(synth, shape), sigmas)
            assert np.array_equal(_bits(got), _bits(want[shape])), shape


def test_the_sweep_replaces_the_prepass(ctx, ife, synth):
    """Four scales are two groups.  Option on: a sweep (booked under `prep`, where the prepass
    stood) and a backward launch per group; option off: one prepass, one full launch per group."""
    img, mask = _inputs(synth, (49, 5, 13))
    counts = {}
    for opt in (1, 0):
        ctx.set_option(ife.OPT_PROFILE, 1)
        try:
            ctx.reset_kernel_times()
            _run(ctx, ife, img, mask, FIVE[:4], OPT_Z_SWEEP=opt)
            ctx.synchronize()
            t = ctx.kernel_times()
        finally:
            ctx.set_option(ife.OPT_PROFILE, 0)
        counts[opt] = (t["prep"][0], t["iir_z"][0], t["iir_x"][0], t["features"][0])
    assert counts[1] == (2, 2, 2, 4) and counts[0] == (1, 2, 2, 4)
