"""The one-process multi-device engine at the edges of its plan (csrc/slab_plan.hpp) and of its
reserve phase: one engine over geometries that grow and shrink, the smallest slabs, and one scale
per chain item.  The test box has one GPU, so the device list names it several times: every slab,
chain item and event of the W-device schedule runs.  Trig mode 0; every result must equal the
one-device call bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _volume(synth, shape, with_mask):
    img = synth.volume_f32(shape, 11)
    mask = None
    if with_mask:
        mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(np.uint8)
        mask[:, :2, :] = 1
    return img, mask


def _same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def _reference(ife, img, mask, sigmas):
    with ife.Context(0) as c:
        c.set_option(ife.OPT_TRIG_MODE, 0)
        fd, diff = c.emphysema_features(img, mask, sigmas), c.differential_features(img, mask, sigmas)
    assert np.abs(fd).max() > 0 and np.abs(diff).max() > 0
    return fd, diff


def test_geometry_grows_and_shrinks_on_one_engine(ife, synth):
    """Buffers are never shrunk and are indexed by the call in flight: S, the fields per scale, the
    item count and the slab sizes all change from call to call, on both paths."""
    small = _volume(synth, (12, 20, 24), False) + ([1.0],)
    large = _volume(synth, (33, 40, 36), True) + ([1.0, 2.0, 4.0],)
    ref_small, ref_large = _reference(ife, *small), _reference(ife, *large)
    with ife.Multi([0, 0, 0]) as m:
        m.set_option(ife.OPT_TRIG_MODE, 0)
        for name, (img, mask, sigmas), (fd, diff) in (("small", small, ref_small), ("large", large, ref_large),
                                                      ("small again", small, ref_small)):
            _same_bits(m.emphysema_features(img, mask, sigmas), fd, name + ": finite differences")
            _same_bits(m.differential_features(img, mask, sigmas), diff, name + ": differential")


def test_smallest_slabs(ife, synth):
    """Two slabs of the minimum 4 planes; 96 lines: one line group of a partial workgroup."""
    img, mask = _volume(synth, (8, 8, 12), True)
    sigmas = [1.0, 2.0]
    fd, diff = _reference(ife, img, mask, sigmas)
    with ife.Multi([0, 0]) as m:
        m.set_option(ife.OPT_TRIG_MODE, 0)
        _same_bits(m.emphysema_features(img, mask, sigmas), fd, "finite differences")
        _same_bits(m.differential_features(img, mask, sigmas), diff, "differential")


def test_one_scale_per_item(ife, synth):
    """Five scales on the differential path over three slabs: five one-scale items per line group
    (320 lines: groups of 256 and 64) and the per-scale bulk phase."""
    img, mask = _volume(synth, (14, 16, 20), True)
    sigmas = [1.0, 1.5, 2.0, 3.0, 4.0]
    with ife.Context(0) as c:
        c.set_option(ife.OPT_TRIG_MODE, 0)
        ref = c.differential_features(img, mask, sigmas)
    assert np.abs(ref).max() > 0
    with ife.Multi([0, 0, 0]) as m:
        m.set_option(ife.OPT_TRIG_MODE, 0)
        _same_bits(m.differential_features(img, mask, sigmas), ref, "differential")
