"""Per-step inputs and references of the slab-engine tests (test_slab.py, test_slab_stream.py).

Step t of a run gets an image and a mask of its own, so that a step which reads a buffer set,
a checkpoint or a state of another step produces wrong bits.  Both are cut from GLOBAL
coordinates: the slabs of one step (with their overlap planes) stitch into that step's whole
volume, which the references are computed on.
"""
import numpy as np

MASK_KINDS = ("labels", "ones", "none")


def step_image(synth, t, shape, z0, nze, i16=False):
    """Planes [z0, z0 + nze) of the image of step t."""
    _, ny, nx = shape
    return (synth.volume_i16 if i16 else synth.volume_f32)((nze, ny, nx), 77 + t, z0=z0)


def step_mask(synth, t, shape, bounds, z0, nze, kind, mdt=np.uint8):
    """Planes [z0, z0 + nze) of the mask of step t, or None (kind "none").

    kind "labels" cycles through three masks with the step:
      0: the two ellipsoids clamped to {0, 1} (and two rows of ones);
      1: thresholded noise, a different pattern every step;
      2: the ellipsoids with no certainty on the two planes either side of every slab cut, and
         none at all from plane 0 up to the first plane above the first cut in half the lines:
         the causal certainty states those lines hand across the first cut are exactly zero.
    """
    nz, ny, nx = shape
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones((nze, ny, nx), mdt)
    assert kind == "labels", kind
    z = np.arange(z0, z0 + nze)
    v = t % 3
    if v == 1:
        m = synth.volume_f32((nze, ny, nx), 1000 + t, z0=z0) > 300
    else:
        m = np.minimum(synth.mask_ellipsoids((nze, ny, nx), z0=z0, nz_total=nz), 1)
        m[:, :2, :] = 1
        if v == 2:
            for c in bounds[1:-1]:
                m[(z >= c - 2) & (z < c + 2)] = 0
            m[z <= bounds[1], : ny // 2] = 0
    return m.astype(mdt)


def whole_step(synth, t, shape, bounds, kind, i16=False):
    """(image, mask) of step t over the whole volume."""
    nz = shape[0]
    return (step_image(synth, t, shape, 0, nz, i16),
            step_mask(synth, t, shape, bounds, 0, nz, kind, np.uint16 if i16 else np.uint8))


def oracle_features(oracle, img, mask, sigma, spacing, layout):
    """The CPU reference of one scale: the oracle's normalized-convolution path with a mask,
    its plain recursive Gaussian (Z, X, Y) and the same features without one."""
    if mask is None:
        S = oracle.smoothing_recursive_gaussian(img.astype(np.float32), sigma, spacing)
        G = oracle.gradient_magnitude(S, spacing)
        F = oracle.eigfeat(oracle.hessian3d(S, spacing))
        res = np.concatenate([S[..., None], G[..., None], F], -1)
    else:
        res = oracle.emphysema_features(img, mask, sigma, spacing)
    return res if layout == 0 else np.ascontiguousarray(np.moveaxis(res, -1, 0))
