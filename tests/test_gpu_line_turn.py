"""The recursive-Gaussian line kernels around the places where a line is cut: its first pair
of register blocks, its last (ragged) one where the sweep turns, the pairs whose checkpoint is
taken three samples in, the tiles of the X pass, and the sibling waves of the paired last
pass.

Axis lengths sit on and around one block and one or two pairs of every block size; line counts
are no multiples of 64, 128 or 256.  Two shapes are long enough for the steady loops of the
default block sizes (a strided axis of 76 samples or more, an X axis of 68 or more).  Every
comparison is bit-exact: the kernels' arithmetic is the reference's, operation for operation.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
CASES = [(1.0, (1, 1, 1)), (2.5, (0.7, 0.8, 1.25))]
SHAPES = [(4, 4, 4), (23, 24, 25), (24, 25, 31), (25, 47, 32), (47, 48, 33), (48, 49, 63),
          (49, 5, 64), (5, 70, 65), (72, 23, 97),
          (100, 77, 40), (77, 100, 160)]  # the steady loops of the default block sizes
BLOCK_SHAPES = [(25, 49, 65), (48, 24, 33)]

_inputs, _refs = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _nc_inputs(synth, shape):
    if shape not in _inputs:
        img = synth.volume_f32(shape, 1234)
        cert = (synth.mask_ellipsoids(shape) > 0).astype(np.float32)
        cert[0, 0, 0] = 1.0
        cert += np.float32(0.25) * (np.arange(cert.size).reshape(shape) % 3 == 0)  # fractional weights
        img.setflags(write=False)
        cert.setflags(write=False)
        _inputs[shape] = (img, cert)
    return _inputs[shape]


def _nc_ref(oracle, synth, shape, sigma, spacing):
    key = (shape, sigma, spacing)
    if key not in _refs:
        img, cert = _nc_inputs(synth, shape)
        ref = oracle.normalized_gaussian_convolution(img, cert, sigma, spacing)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma,spacing", CASES)
def test_whole_convolution_matches_oracle(ctx, oracle, synth, shape, sigma, spacing):
    img, cert = _nc_inputs(synth, shape)
    got = ctx.normalized_gaussian_convolution(img, cert, sigma, spacing)
    assert np.array_equal(_bits(got), _bits(_nc_ref(oracle, synth, shape, sigma, spacing)))


@pytest.mark.parametrize("block", [8, 10, 12, 16])
@pytest.mark.parametrize("shape", BLOCK_SHAPES)
@pytest.mark.parametrize("sigma,spacing", CASES)
def test_every_block_size_turns_alike(ctx, ife, oracle, synth, shape, sigma, spacing, block):
    img, cert = _nc_inputs(synth, shape)
    ctx.set_option(ife.OPT_IIR_BLOCK, block)
    try:
        got = ctx.normalized_gaussian_convolution(img, cert, sigma, spacing)
    finally:
        ctx.set_option(ife.OPT_IIR_BLOCK, 0)
    assert np.array_equal(_bits(got), _bits(_nc_ref(oracle, synth, shape, sigma, spacing)))


def _axis_pass(ctx, torch, fields, shape, spacing, axis, sigmas):
    """One launch of the plain line kernel over `fields` (device tensors); host arrays back."""
    outs = [torch.full(shape, 7.0, dtype=torch.float32, device="cuda") for _ in fields]
    ctx.stage_recursive_gaussian_batch([f.data_ptr() for f in fields], [o.data_ptr() for o in outs],
                                       shape, spacing, axis, sigmas)
    ctx.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("ny", [4, 23, 24, 25, 48, 49, 77])
def test_paired_last_pass_equals_two_fields_divided(ctx, ny):
    """The quotient form on Y against the plain kernel's two fields and the Div rule
    (B != 0 ? A / B : FLT_MAX), three scales at once.  Line counts: less than a wave, one
    wave exactly (its workgroup's other wave pair has no lines), one line more, a workgroup
    and a line, several workgroups.  The denominator has lines of exact zeros (quotient
    FLT_MAX) and lines of ones on the first 64 lines only, so that where the filter keeps a
    line of ones some waves skip the division and their neighbours do not."""
    import torch
    sigmas, spacing = [1.0, 2.0, 4.0], (1.0, 0.8, 1.0)
    for nz, nx in [(1, 5), (1, 64), (5, 13), (3, 43), (4, 75)]:  # nx * nz = 5, 64, 65, 129, 300
        shape = (nz, ny, nx)
        rng = np.random.default_rng(ny * 1000 + nz * nx)
        num = rng.standard_normal(shape).astype(np.float32)
        den = (0.25 + rng.random(shape)).astype(np.float32)
        line = np.arange(nz)[:, None] * nx + np.arange(nx)[None, :]  # the kernel's line index
        dl = np.moveaxis(den, 1, 0)                                  # [ny][nz][nx]
        dl[:, line < 64] = 1.0
        dl[:, line % 7 == 3] = 0.0
        dn, dd = torch.from_numpy(num).cuda(), torch.from_numpy(den).cuda()
        outs = [torch.full(shape, 7.0, dtype=torch.float32, device="cuda") for _ in sigmas]
        ctx.stage_recursive_gaussian_quotient([dn.data_ptr()] * 3, [dd.data_ptr()] * 3,
                                              [o.data_ptr() for o in outs], shape, spacing, 1, sigmas)
        ctx.synchronize()
        fields = _axis_pass(ctx, torch, [dn] * 3 + [dd] * 3, shape, spacing, 1, sigmas + sigmas)
        for j in range(3):
            a, b = fields[j], fields[3 + j]
            with np.errstate(divide="ignore", invalid="ignore"):
                want = np.where(b != 0, a / np.where(b != 0, b, 1), FLT_MAX).astype(np.float32)
            assert (b == 0).any()
            assert np.array_equal(_bits(outs[j].cpu().numpy()), _bits(want)), (shape, sigmas[j])


@pytest.mark.parametrize("nx", [4, 31, 32, 33, 64, 65, 96, 97, 160])
def test_x_pass_is_the_same_for_both_tile_widths(ctx, ife, nx):
    """Six jobs along X with tiles of 32 samples (the default) and of 16: the x history of a
    tile's checkpoint is the tile's own first three samples, at every multiple of the tile
    width.  300 lines: four full waves, which take the pipelined form where rows are
    aligned, and a partial one, which takes the plain form; 7 lines: a single partial wave."""
    import torch
    sigmas, spacing = [1.0, 2.0, 4.0, 1.0, 2.0, 4.0], (0.7, 1.0, 1.0)
    for nz, ny in [(5, 60), (1, 7)]:
        shape = (nz, ny, nx)
        rng = np.random.default_rng(nx * 100 + ny)
        vols = [torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda() for _ in range(2)]
        fields = [vols[0]] * 3 + [vols[1]] * 3
        wide = _axis_pass(ctx, torch, fields, shape, spacing, 0, sigmas)
        ctx.set_option(ife.OPT_IIR_BLOCK, 8)
        try:
            narrow = _axis_pass(ctx, torch, fields, shape, spacing, 0, sigmas)
        finally:
            ctx.set_option(ife.OPT_IIR_BLOCK, 0)
        for j in range(6):
            assert np.array_equal(_bits(wide[j]), _bits(narrow[j])), (shape, j)
            assert np.isfinite(wide[j]).all() and not (wide[j] == 7.0).any()


@pytest.mark.parametrize("axis,shape", [(0, (5, 60, 160)), (1, (3, 100, 100)), (2, (100, 5, 60))])
def test_axis_pass_matches_oracle_in_the_steady_loops(ctx, oracle, axis, shape):
    """One axis at a time, long enough for the steady loops, against the oracle's line filter."""
    import torch
    rng = np.random.default_rng(17 + axis)
    vol = rng.standard_normal(shape).astype(np.float32)
    d = torch.from_numpy(vol).cuda()
    sigmas = [1.0, 2.5, 4.0]
    got = _axis_pass(ctx, torch, [d] * 3, shape, (1.0, 1.0, 1.0), axis, sigmas)
    for g, s in zip(got, sigmas):
        assert np.array_equal(_bits(g), _bits(oracle.recursive_gaussian_axis(vol, axis, s)))


@pytest.mark.parametrize("shape", [(25, 49, 65), (48, 24, 128)])
@pytest.mark.parametrize("certainty", [1.0, 0.0])
def test_constant_lines_on_equals_off(ctx, ife, synth, shape, certainty):
    """All-ones and all-zero certainty; the volume is constant (zeros, ones) on some groups
    of 64 lines of every axis and not on their neighbours."""
    img = synth.volume_f32(shape, 21).copy()
    nz, ny, nx = shape
    img[:3] = 1.0                     # X and Y lines of the first planes
    img[nz - 2:] = 0.0
    img[:, : ny // 2, : nx // 2] = 0.0  # Z lines of a quadrant; X and Y lines in part only
    cert = np.full(shape, certainty, np.float32)
    res = {}
    for opt in (1, 0):
        ctx.set_option(ife.OPT_CONST_LINES, opt)
        try:
            res[opt] = [ctx.normalized_gaussian_convolution(img, cert, s) for s in (1.0, 2.5)]
        finally:
            ctx.set_option(ife.OPT_CONST_LINES, 1)
    for a, b in zip(res[1], res[0]):
        assert np.array_equal(_bits(a), _bits(b))
    if certainty == 0.0:
        assert (res[1][0] == FLT_MAX).all()


def test_same_call_twice_gives_the_same_bits(ctx, synth):
    """Checkpoint areas and parking strips carry nothing from one call to the next, also when
    another shape ran in between."""
    shape = (25, 49, 65)
    img, cert = _nc_inputs(synth, shape)
    first = ctx.normalized_gaussian_convolution(img, cert, 2.5, (0.7, 0.8, 1.25))
    other, ocert = _nc_inputs(synth, (47, 48, 33))
    ctx.normalized_gaussian_convolution(other, ocert, 1.0)
    again = ctx.normalized_gaussian_convolution(img, cert, 2.5, (0.7, 0.8, 1.25))
    assert np.array_equal(_bits(first), _bits(again))


def test_features_through_the_paired_kernel(ctx, oracle, synth):
    from test_gpu_parity import assert_features_close
    shape, sigmas = (25, 49, 65), [1.0, 2.0, 4.0]
    img = synth.volume_f32(shape, synth.SEED_CONFIG[3])
    mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
    got = ctx.emphysema_features(img, mask, sigmas)
    for s, sigma in enumerate(sigmas):
        assert_features_close(got[s], oracle.emphysema_features(img, mask, sigma), mask)
