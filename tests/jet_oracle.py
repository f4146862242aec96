"""numpy oracle of the differential normalized convolution (ife_normalized_convolution_jet,
ife_differential_features): the twenty fields by the CPU oracle's recursive Gaussian, one axis
pass at a time, and the quotient rule of include/ife_hip.h in float64, every operation on its own
and in the stated order.

  cT = float32(image) * float32(certainty)                       (a float multiply)
  F[ox,oy,oz](f) = RG_y^oy(RG_x^ox(RG_z^oz(f)))                  float32 between the passes
  N = F(cT), D = F(c), r = 1 / spacing
  d = D[000]; U = N[000] / d; U_i = (N[i] - U * D[i]) / d
  U_ij = (((N[ij] - U_i * D[j]) - U_j * D[i]) - U * D[ij]) / d
  g_i = U_i * r_i; h_ij = U_ij * (r_i * r_j)

Volumes are [z, y, x]; spacing is (sx, sy, sz); axes are 0 = x, 1 = y, 2 = z.  `oracle` is the
oracle.pyoracle module (the `oracle` fixture)."""
import ctypes as C

import numpy as np

FLT_MAX = np.finfo(np.float32).max
# the ten order triples (ox, oy, oz) in component order: U, x, y, z, xx, xy, xz, yy, yz, zz
TRIPLES = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0),
           (0, 1, 1), (0, 0, 2))
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # (i, j) of components 4..9


def recursive_gaussian_axis_order(oracle, vol, axis_xyz, sigma, spacing, order):
    """One axis pass of ITK's recursive Gaussian of order 0, 1 or 2 (pixel units)."""
    vol = np.ascontiguousarray(vol, np.float32)
    out = np.empty_like(vol)
    nz, ny, nx = vol.shape
    d = oracle.Dims(nx, ny, nz, *[float(s) for s in spacing])
    f32p = C.POINTER(C.c_float)
    rc = oracle.lib().ife_or_recursive_gaussian_axis_order(
        vol.ctypes.data_as(f32p), out.ctypes.data_as(f32p), C.byref(d), C.c_int(axis_xyz),
        C.c_double(sigma), C.c_int(order))
    if rc != 0:
        raise RuntimeError("oracle recursive gaussian failed rc=%d" % rc)
    return out


def fields(oracle, f, sigma, spacing):
    """The ten fields F[t](f), t in TRIPLES order: passes z, x, y."""
    rg = lambda v, axis, order: recursive_gaussian_axis_order(oracle, v, axis, sigma, spacing, order)
    z = [rg(f, 2, k) for k in range(3)]
    x = {(ox, oz): rg(z[oz], 0, ox) for oz in range(3) for ox in range(3 - oz)}
    return [rg(x[(ox, oz)], 1, oy) for (ox, oy, oz) in TRIPLES]


def jet64(oracle, image, certainty, sigma, spacing=(1.0, 1.0, 1.0)):
    """(U, g[3], h[6]) in float64; float64(FLT_MAX) everywhere the stored float D[000] is 0."""
    image = np.ascontiguousarray(image, np.float32)
    certainty = np.ascontiguousarray(certainty, np.float32)
    ct = image * certainty   # float32 * float32, rounded to float32
    N = [a.astype(np.float64) for a in fields(oracle, ct, sigma, spacing)]
    D = [a.astype(np.float64) for a in fields(oracle, certainty, sigma, spacing)]
    r = [np.float64(1.0) / np.float64(s) for s in spacing]
    zero = D[0] == 0.0
    with np.errstate(all="ignore"):
        d = D[0]
        U = N[0] / d
        U1 = [(N[1 + i] - U * D[1 + i]) / d for i in range(3)]
        g = [U1[i] * r[i] for i in range(3)]
        h = []
        for p, (i, j) in enumerate(PAIRS):
            t = N[4 + p] - U1[i] * D[1 + j]
            t = t - U1[j] * D[1 + i]
            t = t - U * D[4 + p]
            h.append((t / d) * (r[i] * r[j]))
    fix = lambda a: np.where(zero, np.float64(FLT_MAX), a)
    return fix(U), [fix(a) for a in g], [fix(a) for a in h]


def jet(oracle, image, certainty, sigma, spacing=(1.0, 1.0, 1.0)):
    """(nz, ny, nx, 10) float32: U, g_x, g_y, g_z, h_xx, h_xy, h_xz, h_yy, h_yz, h_zz."""
    U, g, h = jet64(oracle, image, certainty, sigma, spacing)
    with np.errstate(over="ignore"):
        return np.stack([U] + g + h, -1).astype(np.float32)


def features(oracle, image, mask, sigma, spacing=(1.0, 1.0, 1.0), trig_mode=0):
    """(nz, ny, nx, 8) float32 in the order of IFE_FEATURE_NAMES; mask None = all ones, its value
    is the certainty weight and every component is zero where it is zero."""
    image = np.asarray(image).astype(np.float32)
    cert = np.ones(image.shape, np.float32) if mask is None else np.asarray(mask).astype(np.float32)
    U, g, h = jet64(oracle, image, cert, sigma, spacing)
    with np.errstate(all="ignore"):
        G = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).astype(np.float32)
        h32 = np.stack(h, -1).astype(np.float32)
        out = np.concatenate([U.astype(np.float32)[..., None], G[..., None],
                              oracle.eigfeat(h32, trig_mode)], -1)
    if mask is not None:
        out = np.where((np.asarray(mask) != 0)[..., None], out, np.float32(0.0))
    return np.ascontiguousarray(out, np.float32)
