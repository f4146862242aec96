"""The sampling definitions of include/ife_hip.h ("sampling") in numpy and Python integers,
written from the definitions and not from the C++: Philox4x32-10, the rank of a draw, the
admissible voxels of a set, the draws and their boxes, and the box gather."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four 32-bit words, key: two; returns the four output words."""
    c = [int(v) & MASK32 for v in counter]
    k = [int(v) & MASK32 for v in key]
    for rnd in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK32]
        if rnd < 9:
            k = [(k[0] + W0) & MASK32, (k[1] + W1) & MASK32]
    return c


def rank(seed, stream, k, n):
    """floor(u * n / 2^64) of draw k (any non-negative integer, taken mod 2^64) of a stream."""
    k &= (1 << 64) - 1
    o = philox4x32_10((k & MASK32, k >> 32, stream & MASK32, 0), (seed & MASK32, (seed >> 32) & MASK32))
    return ((o[0] + (o[1] << 32)) * n) >> 64


def ranks(seed, stream, k_array, n):
    """rank() of every draw number of k_array (non-negative integers, each taken mod 2^64) at once:
    an int64 array of k_array's shape.  The ten rounds run on uint64 arrays of 32-bit words, whose
    products with the 32-bit multipliers fit 64 bits; the final * n >> 64 is done in Python
    integers, as in rank()."""
    k = np.asarray(k_array)
    if k.dtype != np.uint64:   # Python integers beyond 2^64 - 1 included
        k = np.array([int(v) & ((1 << 64) - 1) for v in k.reshape(-1)], np.uint64).reshape(k.shape)
    shape, k = k.shape, k.reshape(-1)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    c = [k & m32, k >> s32, np.full(k.shape, int(stream) & MASK32, np.uint64), np.zeros(k.shape, np.uint64)]
    key = [int(seed) & MASK32, (int(seed) >> 32) & MASK32]
    for rnd in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(key[0]), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(key[1]), p0 & m32]
        if rnd < 9:
            key = [(key[0] + W0) & MASK32, (key[1] + W1) & MASK32]
    u = c[0] + (c[1] << s32)
    n = int(n)
    return np.array([(int(v) * n) >> 64 for v in u], np.int64).reshape(shape)


def fits(shape_zyx, size_xyz):
    """Boolean (z, y, x) volume: the box of size_xyz around the voxel lies inside the volume."""
    out = np.ones(shape_zyx, bool)
    for axis, s in zip((2, 1, 0), size_xyz):
        n, h = shape_zyx[axis], s // 2
        i = np.arange(n)
        ok = (i - h >= 0) & (i - h + s <= n)
        out &= ok.reshape([-1 if a == axis else 1 for a in range(3)])
    return out


def set_predicates(mask, values, per_value):
    """The membership volume of every set."""
    values = list(values)
    if not values:
        return [mask != 0]
    if not per_value:
        return [np.isin(mask, values)]
    return [mask == v for v in values]


def admissible(mask, size_xyz=(1, 1, 1), values=(), per_value=False):
    """A_j of every set: increasing linear indices."""
    f = fits(mask.shape, size_xyz)
    return [np.flatnonzero(p & f) for p in set_predicates(mask, values, per_value)]


def sample_positions(mask, n_draws, size_xyz=(1, 1, 1), values=(), per_value=False, seed=0, stream=0, first_draw=0):
    """(positions (sets, n_draws) int64, n_admissible (sets,)); a ValueError naming the set where
    one is empty and draws are asked for."""
    sets = admissible(mask, size_xyz, values, per_value)
    counts = np.array([len(a) for a in sets], np.int64)
    out = np.empty((len(sets), n_draws), np.int64)
    # the draw numbers modulo 2^64 (uint64 arrays wrap)
    k = np.full(n_draws, int(first_draw) & ((1 << 64) - 1), np.uint64) + np.arange(n_draws, dtype=np.uint64)
    for j, a in enumerate(sets):
        if n_draws and len(a) == 0:
            raise ValueError("set %d is empty" % j)
        if n_draws:
            out[j] = a[ranks(seed, stream + j, k, len(a))]
    return out, counts


def boxes_of(positions, shape_zyx, size_xyz):
    """(..., 6) boxes {x - hx, y - hy, z - hz, sx, sy, sz} of linear indices."""
    nz, ny, nx = shape_zyx
    sx, sy, sz = size_xyz
    p = np.asarray(positions, np.int64)
    x, y, z = p % nx, (p // nx) % ny, p // (nx * ny)
    size = [np.full(p.shape, s, np.int64) for s in size_xyz]
    return np.stack([x - sx // 2, y - sy // 2, z - sz // 2] + size, axis=-1)


def random_rois(mask, n_draws, size_xyz, **kw):
    pos, counts = sample_positions(mask, n_draws, size_xyz, **kw)
    return boxes_of(pos, mask.shape, size_xyz), counts


def extract_rois(src, rois):
    rois = np.asarray(rois, np.int64).reshape(-1, 6)
    return np.stack([src[z:z + sz, y:y + sy, x:x + sx] for x, y, z, sx, sy, sz in rois])


def roi_info_lines(rois):
    """The lines of a .ROIInfo file: [x, y, z][sx, sy, sz]."""
    return ["[%d, %d, %d][%d, %d, %d]" % tuple(int(v) for v in r) for r in np.asarray(rois).reshape(-1, 6)]
