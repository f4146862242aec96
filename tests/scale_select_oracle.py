"""A numpy restatement of ife_scale_select (include/ife_hip.h "scale selection"): the measures and
the fold over scales from a [S][...][8] feature array.  The checker of the tests, never the thing
under test.  IFE_SS_LAPLACIAN is evaluated in float32, as the library evaluates it (one float
product, exact); the three Frangi kinds in float64 from the float32 a_k, the float32 weight and the
float32 reciprocals, so that what a test sees between this and the device is the float arithmetic
of the kernel alone."""
import math

import numpy as np

LAPLACIAN, TUBE, PLATE, BLOB = 0, 1, 2, 3
MAX_MEASURES, MAX_SIGMAS = 4, 255
OK, ARG = 0, 1
NONE = 255


def measure(kind, polarity=1, gamma=1.0, alpha=0.5, beta=0.5, c=1.0):
    return dict(kind=kind, polarity=polarity, gamma=gamma, alpha=alpha, beta=beta, c=c)


def weight(sigma, gamma):
    """w_s = (float)pow((double)sigma, 2 * (double)gamma) of float32 sigma and gamma."""
    return np.float32(math.pow(float(np.float32(sigma)), 2.0 * float(np.float32(gamma))))


def reciprocal(v):
    """1 / (2 v^2) in double of a float32 v, rounded to float32."""
    v = float(np.float32(v))
    return np.float32(1.0 / (2.0 * v * v))


def _positive_finite(v):
    v = np.float32(v)
    return bool(v > 0 and np.isfinite(v))


def check(n_measures, n_sigmas, measures):
    """The verdict of the library's argument checks: (OK | ARG, index of the offending measure or
    -1)."""
    if not 1 <= n_measures <= MAX_MEASURES:
        return ARG, -1
    if n_sigmas > MAX_SIGMAS:
        return ARG, -1
    if measures is None:
        return ARG, -1
    for k, m in enumerate(measures[:n_measures]):
        if m["kind"] not in (LAPLACIAN, TUBE, PLATE, BLOB) or m["polarity"] not in (1, -1):
            return ARG, k
        g = np.float32(m["gamma"])
        if not (g >= 0 and np.isfinite(g)):
            return ARG, k
        if m["kind"] != LAPLACIAN and not all(_positive_finite(m[n]) for n in ("alpha", "beta", "c")):
            return ARG, k
    return OK, -1


def responses(features, sigmas, m):
    """R[s] of one measure for every scale: float32 for LAPLACIAN, float64 for the Frangi kinds.
    features: [S][...][8]."""
    features = np.asarray(features, np.float32)
    sign = np.float32(-1.0 if m["polarity"] > 0 else 1.0)
    out = []
    with np.errstate(all="ignore"):
        for s, sigma in enumerate(sigmas):
            w = weight(sigma, m["gamma"])
            f = features[s]
            if m["kind"] == LAPLACIAN:
                out.append(sign * (w * f[..., 5]))
                continue
            a1, a2, a3 = w * f[..., 4], w * f[..., 3], w * f[..., 2]      # float32 products
            s1, s2, s3 = sign * a1 > 0, sign * a2 > 0, sign * a3 > 0
            ka, kb, kc = (float(reciprocal(m[n])) for n in ("alpha", "beta", "c"))
            a1, a2, a3 = a1.astype(np.float64), a2.astype(np.float64), a3.astype(np.float64)
            ra2 = a2 * a2 / (a3 * a3)
            rb2 = np.where(a2 == 0, 0.0, a1 * a1 / np.abs(a2 * a3))
            A, B = np.exp(-ra2 * ka), np.exp(-rb2 * kb)
            C = 1.0 - np.exp(-(a1 * a1 + a2 * a2 + a3 * a3) * kc)
            if m["kind"] == TUBE:
                r, counts = (1.0 - A) * B * C, s2 & s3
            elif m["kind"] == PLATE:
                r, counts = A * B * C, s3
            else:
                r, counts = (1.0 - A) * (1.0 - B) * C, s1 & s2 & s3
            out.append(np.where(counts, r, 0.0))
    return np.stack(out)


def fold(R):
    """(best, index) over the scales of R[s] in order: best = 0 and index = 255, replaced only by a
    strictly larger response, so the first of equal scales wins and a NaN never does."""
    best = np.zeros(R.shape[1:], R.dtype)
    index = np.full(R.shape[1:], NONE, np.uint8)
    with np.errstate(invalid="ignore"):
        for s in range(R.shape[0]):
            wins = R[s] > best
            best = np.where(wins, R[s], best)
            index = np.where(wins, np.uint8(s), index)
    return best, index


def scale_select(features, sigmas, measures):
    """(response [M][...], index [M][...] uint8); the response is float32 for LAPLACIAN rows and
    holds the float64 maximum rounded to float32 for the others (compare those with a tolerance,
    or use responses() and fold() directly)."""
    resp, idx = [], []
    for m in measures:
        b, i = fold(responses(features, sigmas, m))
        resp.append(b.astype(np.float32))
        idx.append(i)
    return np.stack(resp), np.stack(idx)
