"""ife_stage_jet_features: everything of ife_differential_features behind its Z level.  Fed with
the six Z-level fields that ife_stage_recursive_gaussian_order makes of cT and c along z, it
must give what the one-device call gives on the same volume bit for bit: both layouts, both mask
widths, no mask; (9, 10, 11) has 990 voxels (n % 4 = 2: the scalar tail of the pointwise pass)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPACING = (0.7, 1.3, 2.0)
SIGMA = 1.5


def _inputs(synth, shape, mask_kind):
    img = synth.volume_f32(shape, 23)
    labels = synth.mask_ellipsoids(shape)
    labels[:, :2, :] = 1
    if mask_kind == "none":
        return img, None
    if mask_kind == "u8":
        return img, np.minimum(labels, 1).astype(np.uint8)
    return img, labels.astype(np.uint16)   # {0, 1, 2}: the label value is the certainty weight


@pytest.mark.parametrize("mask_kind", ["u8", "u16", "none"])
@pytest.mark.parametrize("layout_name", ["INTERLEAVED", "PLANAR"])
@pytest.mark.parametrize("shape", [(9, 10, 11), (12, 20, 24)])
def test_stage_jet_features_equal_the_one_device_call(ife, ctx, synth, shape, layout_name, mask_kind):
    import torch
    layout = getattr(ife, layout_name)
    img, mask = _inputs(synth, shape, mask_kind)
    d_img = torch.from_numpy(img).cuda()
    if mask is None:
        d_mask, mdt, p_mask = None, ife.U8, None
    elif mask.dtype == np.uint8:
        d_mask, mdt = torch.from_numpy(mask).cuda(), ife.U8
        p_mask = d_mask.data_ptr()
    else:
        d_mask, mdt = torch.from_numpy(mask.view(np.int16)).cuda(), ife.U16
        p_mask = d_mask.data_ptr()
    # the sources: cT = float(image) * float(mask), c = float(mask) (the constant one without a mask)
    ct = torch.empty(shape, dtype=torch.float32, device="cuda")
    cf = torch.ones(shape, dtype=torch.float32, device="cuda")
    ctx.stage_prepare(d_img.data_ptr(), ife.F32, p_mask, mdt, shape, ct.data_ptr(),
                      cf.data_ptr() if mask is not None else None)
    zf = [torch.empty(shape, dtype=torch.float32, device="cuda") for _ in range(6)]
    for s, src in enumerate((ct, cf)):
        for k in range(3):
            ctx.stage_recursive_gaussian_order(src.data_ptr(), zf[3 * s + k].data_ptr(), shape, SPACING, 2, SIGMA, k)
    oshape = shape + (8,) if layout == ife.INTERLEAVED else (8,) + shape
    got = torch.full(oshape, float("nan"), dtype=torch.float32, device="cuda")
    ctx.stage_jet_features([t.data_ptr() for t in zf], p_mask, mdt, shape, SPACING, SIGMA, got.data_ptr(), layout)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = torch.full(oshape, float("nan"), dtype=torch.float32, device="cuda")
    ctx.differential_features_device(d_img.data_ptr(), ife.F32, p_mask, mdt, shape, SPACING, [SIGMA],
                                     want.data_ptr(), layout)
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    assert not np.isnan(want).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(want).max() > 0


def test_stage_jet_features_refuses_bad_arguments(ife, ctx):
    import torch
    shape = (4, 8, 8)
    z = torch.zeros(shape, dtype=torch.float32, device="cuda")
    out = torch.zeros(shape + (8,), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        ctx.stage_jet_features([z.data_ptr()] * 5, None, ife.U8, shape, SPACING, SIGMA, out.data_ptr())
    with pytest.raises(ife.IfeError) as e:      # a missing field
        ctx.stage_jet_features([z.data_ptr()] * 5 + [0], None, ife.U8, shape, SPACING, SIGMA, out.data_ptr())
    assert e.value.code == ife.E_ARG
    with pytest.raises(ife.IfeError) as e:      # interleaved output off the 16-byte grid
        ctx.stage_jet_features([z.data_ptr()] * 6, None, ife.U8, shape, SPACING, SIGMA, out.data_ptr() + 4)
    assert e.value.code == ife.E_ARG
    with pytest.raises(ife.IfeError) as e:      # three voxels along x
        ctx.stage_jet_features([z.data_ptr()] * 6, None, ife.U8, (4, 8, 3), SPACING, SIGMA, out.data_ptr())
    assert e.value.code == ife.E_SIZE
