"""numpy restatement of the three definitions of the census and coverage calls
(include/ife_hip.h "census and coverage"): the value census of a float32 array on canonicalised
bits, the inclusive threshold, and the coverage of a mask by a growing list of boxes, painted box by
box into a boolean volume.  Also the lines the ImageBrowser tool prints from them, formatted with
%g, which is what C++'s operator<< gives floats and doubles at its default precision of 6."""
import numpy as np

# the partial sums of nSamplesPerRound of the reference's tools/ImageBrowser.cxx:70
SAMPLES_PER_ROUND = (10, 10, 10, 10, 10, 50, 100, 100, 100, 100, 500, 1000)
ROUND_ENDS = (10, 20, 30, 40, 50, 100, 200, 300, 400, 500, 1000, 2000)
COMMANDS = "'q' : quit\n'i' : Info about image shape\n's' : Summary statistics\n'r' : ROI overlap estimation\n"


def _bits(values):
    return np.ascontiguousarray(values, np.float32).reshape(-1).view(np.uint32)


def is_nan_bits(bits):
    return (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def order_image(bits):
    """The order-preserving integer image of non-NaN float bits; -0 and +0 share 0."""
    mag = (bits & np.uint32(0x7fffffff)).astype(np.int64)
    return np.where(bits >> np.uint32(31), -mag, mag)


def value_census(values):
    """(uniq float32 ascending, counts uint32, n_nan): NaNs left out and counted, -0 as +0, any
    other two elements one value iff their bits are equal."""
    bits = _bits(values)
    nan = is_nan_bits(bits)
    kept = bits[~nan].copy()
    kept[kept == np.uint32(0x80000000)] = 0
    # distinct bit patterns, ordered as floats: order_image is one-to-one on canonical bits
    ub, counts = np.unique(kept, return_counts=True)
    order = np.argsort(order_image(ub), kind="stable")
    return ub[order].view(np.float32), counts[order].astype(np.uint32), int(nan.sum())


def threshold_mask(image, low, high):
    """(mask uint8, count): 1 where low <= image <= high by the integer images, 0 at NaNs."""
    image = np.ascontiguousarray(image, np.float32)
    bits = _bits(image)
    lo, hi = (int(order_image(_bits(np.float32(v)))[0]) for v in (low, high))
    img = order_image(bits)
    mask = (~is_nan_bits(bits) & (lo <= img) & (img <= hi)).astype(np.uint8).reshape(image.shape)
    return mask, int(mask.sum())


def roi_coverage(mask, rois, round_ends):
    """(visited, hits, region_size) of a (z, y, x) mask, boxes (n, 6) {x, y, z, sx, sy, sz} and
    cumulative round ends: a boolean volume painted box by box and never cleared."""
    fg = np.asarray(mask) != 0
    rois = np.asarray(rois, np.int64).reshape(-1, 6)
    seen = np.zeros(fg.shape, bool)
    visited, hits, done = [], [], 0
    for end in round_ends:
        for x, y, z, sx, sy, sz in rois[done:end]:
            seen[z:z + sz, y:y + sy, x:x + sx] = True
        done = max(done, end)
        visited.append(int(seen.sum()))
        hits.append(int((seen & fg).sum()))
    return np.array(visited, np.int64), np.array(hits, np.int64), int(fg.sum())


def roi_coverage_brute(mask, rois, round_ends):
    """The same numbers voxel by voxel: a voxel counts in round r when some box before
    round_ends[r] holds it."""
    fg = np.asarray(mask) != 0
    rois = np.asarray(rois, np.int64).reshape(-1, 6)
    nz, ny, nx = fg.shape
    first = np.full(fg.shape, len(rois), np.int64)   # the first box that holds the voxel
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                for k, (x0, y0, z0, sx, sy, sz) in enumerate(rois):
                    if x0 <= x < x0 + sx and y0 <= y < y0 + sy and z0 <= z < z0 + sz:
                        first[z, y, x] = k
                        break
    visited = [int((first < e).sum()) for e in round_ends]
    hits = [int(((first < e) & fg).sum()) for e in round_ends]
    return np.array(visited, np.int64), np.array(hits, np.int64), int(fg.sum())


# ---- what the tool prints -----------------------------------------------------------------------------
def g(v):
    return "%g" % float(v)


def census_lines(uniq, counts):
    """The two lines of the `s` command: the bins (old, val] from -1e12 on and (old, inf), then the
    counts with the trailing bin's 0."""
    old, edges = np.float32(-1e12), ""
    for v in uniq:
        edges += "(%s,%s]\t|\t" % (g(old), g(v))
        old = v
    edges += "(%s,inf)\t|\t" % g(old)
    return [edges, "".join("%d\t|\t" % c for c in list(counts) + [0])]


def coverage_lines(visited, hits, region_size, round_ends=ROUND_ENDS):
    return ["Visited %d voxels. %d ROIs overlap %d/%d = %s" % (v, e, h, region_size, g(h / region_size))
            for v, h, e in zip(visited, hits, round_ends)]
