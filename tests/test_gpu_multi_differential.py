"""ife_multi_differential_features: the differential feature path over the Z-slab engine.  The
test box has one GPU, so the device list names it several times: every slab, chain item and event
of the W-device schedule runs.  The result must equal Context.differential_features bit for bit;
one case is also held against the numpy oracle of the path, so that the test does not rest on the
one-device call alone."""
import os
import sys

import numpy as np
import pytest

from oracle.parity import assert_eig_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jet_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_MODE0 = 1e-6   # the project's mode-0 bar for this path (tests/test_gpu_differential.py)

CASES = {
    1: (1, (20, 24, 28), np.float32, np.uint8, [1.0, 2.0], (1.0, 1.0, 1.0)),
    2: (2, (33, 40, 36), np.float32, np.uint8, [1.0, 2.0, 4.0], (1.0, 1.0, 1.0)),
    3: (3, (29, 24, 70), np.int16, np.uint16, [1.5, 3.0], (0.7, 0.8, 1.25)),
    8: (8, (37, 20, 24), np.float32, None, [1.0, 2.0], (1.0, 1.0, 1.0)),   # slabs of 5 and 4 planes; no mask
}


def _volume(synth, shape, dt, mdt):
    img = synth.volume_i16(shape, 9) if dt == np.int16 else synth.volume_f32(shape, 9)
    mask = None
    if mdt is not None:
        mask = np.minimum(synth.mask_ellipsoids(shape), 1).astype(mdt)
        mask[:, :2, :] = 1
    return img, mask


def _same_bits(a, b, what=""):
    assert a.shape == b.shape, what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


@pytest.mark.parametrize("case", sorted(CASES))
def test_engine_equals_one_device(ife, synth, case):
    world, shape, dt, mdt, sigmas, spacing = CASES[case]
    img, mask = _volume(synth, shape, dt, mdt)
    with ife.Context(0) as c:
        c.set_option(ife.OPT_TRIG_MODE, 0)
        ref = c.differential_features(img, mask, sigmas, spacing)
        ref_planar = c.differential_features(img, mask, sigmas, spacing, layout=ife.PLANAR)
    assert np.abs(ref).max() > 0
    with ife.Multi([0] * world) as m:
        m.set_option(ife.OPT_TRIG_MODE, 0)
        _same_bits(m.differential_features(img, mask, sigmas, spacing), ref, "first call")
        _same_bits(m.differential_features(img, mask, sigmas, spacing), ref, "buffers and streams reused")
        _same_bits(m.differential_features(img, mask, sigmas, spacing, layout=ife.PLANAR), ref_planar, "planar")
        _same_bits(m.differential_features(img, mask, sigmas, spacing, layout=ife.PLANAR), ref_planar, "planar again")


def test_engine_equals_one_device_in_the_default_trig_mode(ife, synth):
    world, shape, dt, mdt, sigmas, spacing = CASES[2]
    img, mask = _volume(synth, shape, dt, mdt)
    with ife.Context(0) as c:
        c.set_option(ife.OPT_TRIG_MODE, 2)
        ref = c.differential_features(img, mask, sigmas, spacing)
    with ife.Multi([0] * world) as m:
        m.set_option(ife.OPT_TRIG_MODE, 2)
        _same_bits(m.differential_features(img, mask, sigmas, spacing), ref)


def test_engine_against_the_numpy_oracle(ife, synth, oracle):
    world, shape, dt, mdt, sigmas, spacing = CASES[3]
    img, mask = _volume(synth, shape, dt, mdt)
    with ife.Multi([0] * world) as m:
        m.set_option(ife.OPT_TRIG_MODE, 0)
        got = m.differential_features(img, mask, sigmas, spacing)
    for s, sigma in enumerate(sigmas):
        ref = jet_oracle.features(oracle, img, mask, sigma, spacing)
        what = "sigma %g" % sigma
        np.testing.assert_array_equal(got[s][..., 0], ref[..., 0], what + ": S")
        np.testing.assert_array_equal(got[s][..., 1], ref[..., 1], what + ": G")
        assert_eig_parity(got[s], ref, TOL_MODE0, what)
        assert (got[s][mask == 0].view(np.uint32) == 0).all(), what + ": not zero outside the mask"


def test_stream_yields_what_the_blocking_call_returns(ife, synth):
    world, shape, dt, mdt, sigmas, spacing = CASES[3]
    img, mask = _volume(synth, shape, dt, mdt)
    with ife.Multi([0, 0, 0]) as m:
        m.set_option(ife.OPT_TRIG_MODE, 0)
        want = m.differential_features(img, mask, sigmas, spacing)
        got = list(m.differential_features_stream(img, mask, sigmas, spacing))
        assert len(got) == len(sigmas)
        for k, g in enumerate(got):
            _same_bits(g, want[k], "scale %d" % k)
        # a fetch without a begin, and a blocking call inside a streaming one
        out = np.empty(shape + (8,), np.float32)
        assert m._lib.ife_multi_emphysema_features_fetch(m._h, 0, out.ctypes.data) == ife.E_STATE
        gen = m.differential_features_stream(img, mask, sigmas, spacing)
        next(gen)
        with pytest.raises(ife.IfeError) as e:
            m.differential_features(img, mask, sigmas[:1], spacing)
        assert e.value.code == ife.E_STATE
        gen.close()   # runs _end
        _same_bits(m.differential_features(img, mask, sigmas[:1], spacing)[0], want[0], "after the stream")


def test_one_engine_runs_both_paths_in_turn(ife, synth):
    world, shape, dt, mdt, sigmas, spacing = CASES[2]
    img, mask = _volume(synth, shape, dt, mdt)
    with ife.Context(0) as c:
        c.set_option(ife.OPT_TRIG_MODE, 0)
        ref_diff = c.differential_features(img, mask, sigmas, spacing)
        ref_fd = c.emphysema_features(img, mask, sigmas, spacing)
    with ife.Multi([0] * 3) as m:
        m.set_option(ife.OPT_TRIG_MODE, 0)
        _same_bits(m.differential_features(img, mask, sigmas, spacing), ref_diff, "differential")
        _same_bits(m.emphysema_features(img, mask, sigmas, spacing), ref_fd, "finite differences")
        _same_bits(m.differential_features(img, mask, sigmas, spacing), ref_diff, "differential again")


def test_thin_slabs_are_refused(ife):
    with ife.Multi([0, 0, 0]) as m:
        with pytest.raises(ife.IfeError) as e:
            m.differential_features(np.zeros((8, 8, 8), np.float32), None, [1.0])   # 8 planes over 3 devices
        assert e.value.code == ife.E_SIZE and "4 planes" in str(e.value)
