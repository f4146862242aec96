"""The three box passes of the dense bag and of the dense label mode (dense_box_x_kernel,
dense_box_y_kernel, dense_box_z_kernel of csrc/dense_kernels.hpp, label_mode_z_kernel of
csrc/labels_kernels.hpp) at the shapes where they take another branch: window rows of three to five
64-voxel pieces, marches of more than one chunk, counters at their last value, and more work items
than one grid holds.

Every case asserts, in its own arithmetic, the threshold it crosses (piece count, chunk size, chunk
count and last-chunk length, work items against 2^20 waves), so that a later change of a constant
makes the test say that it no longer covers the edge.  The checkers are oracle.roi_histograms on
the box list of the generator's rule (histograms) and labels_oracle.dense_labels (labels); at small
sizes labels_oracle.roi_labels, box by box, is the second witness.  Everything is integer counting:
results must be EQUAL.

Not reached: the 32-bit limit of the z sum (sx*sy*sz = 2^32 - 1 needs a volume of 4 Gi voxels; no
test of a few seconds stores more than 131 070 there).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import labels_oracle as L  # noqa: E402
from test_gpu_dense_bag import dense_boxes  # noqa: E402  (the generator's rule in numpy)

pytestmark = pytest.mark.gpu

RULES = [((), -1), ((0,), -1), ((0, 255), 7)]
LABEL_SET = np.array([0, 1, 2, 7, 255], np.uint8)
GRID_WAVES = 1 << 20        # csrc/dense_capi.inc dense_blocks: at most 1 << 18 workgroups of four waves
PER_BOX = 2500              # regions the box-by-box Python oracle is asked about per case


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def hist_inputs(seed, shape, ncomp=2, n_edges=5, gen_on=0.75):
    """One-decimal values (so that some land on edges), a counting mask of 0 / 1 / 2 and a random
    generating mask of another dtype and value."""
    rng = np.random.default_rng(seed)
    feat = np.round(rng.normal(0, 3, shape + (ncomp,)), 1).astype(np.float32)
    edges = np.sort(np.round(rng.normal(0, 3, (ncomp, n_edges)), 1).astype(np.float32), axis=1)
    mask = rng.integers(0, 3, shape).astype(np.uint8)
    gen = (rng.random(shape) < gen_on).astype(np.uint16) * 300
    return feat, edges, mask, gen


def hist_want(oracle, feat, edges, mask, gen, size):
    boxes = dense_boxes(gen, size)
    want, _ = oracle.roi_histograms(feat, np.minimum(mask, 1), boxes, edges)
    return boxes, want


def assert_hist(ctx, h):
    got = ctx.dense_roi_histograms(h["feat"], h["mask"], h["size"], h["edges"], gen_mask=h["gen"])
    assert got.dtype == np.uint32 and got.shape == h["want"].shape
    assert np.array_equal(got, h["want"])


def label_wants(lab, gen, size):
    return {rule: L.dense_labels(lab, gen, size, *rule) for rule in RULES}


def assert_labels(ctx, lab, gen, size, wants):
    for rule, want in wants.items():
        got = ctx.dense_roi_labels(lab, gen, size, *rule)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), rule


# ---- 1. wide x windows: rows of three, four and five pieces ----------------------------------------
# dense_box_x_kernel reads a window row in npieces = (64 + sx - 1 + 63) / 64 pieces of 64 voxels and
# keeps a bit mask per piece and lane.
WIDE_SHAPE = (3, 4, 300)            # five row segments, the last one of 44 voxels
WIDE = [(65, 2), (66, 3), (129, 3), (130, 4), (193, 4), (194, 5), (255, 5)]      # sx, pieces
WIDE_SEED = 0


def run_labels(seed, shape, longest=90, sprinkle=40):
    """Every row its own runs along x of random lengths 1..longest, drawn from LABEL_SET, and single
    voxels of LABEL_SET on top."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    lab = np.empty(shape, np.uint8)
    for row in lab.reshape(-1, nx):
        x = 0
        while x < nx:
            n = int(rng.integers(1, longest + 1))
            row[x:x + n] = LABEL_SET[rng.integers(0, len(LABEL_SET))]
            x += n
    pos = rng.choice(lab.size, sprinkle, replace=False)
    lab.reshape(-1)[pos] = LABEL_SET[rng.integers(0, len(LABEL_SET), sprinkle)]
    return lab


@pytest.fixture(scope="module")
def wide(oracle):
    """Inputs once; per box width the wanted histograms and labels.  Never written to."""
    nz, ny, nx = WIDE_SHAPE
    assert (nx + 63) // 64 == 5 and nx % 64 == 44
    feat, edges, mask, gen = hist_inputs(201, WIDE_SHAPE)
    lab = run_labels(WIDE_SEED, WIDE_SHAPE)
    assert set(np.unique(lab)) == set(LABEL_SET.tolist())
    all_on = np.ones(WIDE_SHAPE, np.uint8)
    case = {"feat": feat, "edges": edges, "mask": mask, "gen": gen, "lab": lab, "all_on": all_on, "hist": {},
            "labels": {}}
    frozen(feat, edges, mask, gen, lab, all_on)
    for sx, _ in WIDE:
        size = (sx, 2, 2)
        boxes, want = hist_want(oracle, feat, edges, mask, gen, size)
        assert 0 < len(boxes) < (nx - sx + 1) * 3 * 2 and want.any()
        wants = label_wants(lab, all_on, size)
        boxes_all = dense_boxes(all_on, size)
        assert len(boxes_all) == (nx - sx + 1) * 3 * 2 and 276 <= len(boxes_all) <= 1416
        for rule, w in wants.items():
            assert np.array_equal(w, L.roi_labels(lab, boxes_all, *rule)), (sx, rule)
        tied = L.dense_ties(lab, all_on, size)
        assert tied.any() and not tied.all(), sx           # the smallest of equals is asked for, and not always
        assert len(set(wants[RULES[0]].tolist())) >= 3
        frozen(want, *wants.values())
        case["hist"][sx] = dict(feat=feat, edges=edges, mask=mask, gen=gen, size=size, want=want)
        case["labels"][sx] = wants
    return case


@pytest.mark.parametrize("sx,pieces", WIDE)
def test_wide_windows_histograms(ctx, wide, sx, pieces):
    assert (sx + 126) // 64 == pieces and sx <= 255
    assert_hist(ctx, wide["hist"][sx])


@pytest.mark.parametrize("sx,pieces", WIDE)
def test_wide_windows_labels(ctx, wide, sx, pieces):
    assert (sx + 126) // 64 == pieces and sx <= 255
    assert_labels(ctx, wide["lab"], wide["all_on"], (sx, 2, 2), wide["labels"][sx])


# ---- 2. marches of more than one chunk ---------------------------------------------------------------
# csrc/dense_capi.inc dense_box_passes (and dense_label_passes of csrc/labels_capi.inc): a wave of
# the y or z pass marches chunk = min(max(2 s, 64), n - s + 1) outputs, then another wave starts at
# o0 = ch * chunk with a start-up sum of its own.
def march(n, s):
    """(chunk, chunks, outputs of the last chunk) of a march over n voxels with a window of s."""
    nout = n - s + 1
    chunk = min(max(2 * s, 64), nout)
    nch = -(-nout // chunk)
    return chunk, nch, nout - (nch - 1) * chunk


# volume (nz, ny, nx), box (sx, sy, sz), march along y, march along z, seed of the labels
MARCHES = [
    ((5, 99, 9), (3, 33, 3), (66, 2, 1), (3, 1, 3), 1),         # y: chunk 2 sy, the last chunk one row
    ((6, 131, 9), (3, 3, 3), (64, 3, 1), (4, 1, 4), 0),         # y: three chunks, the last one row
    ((6, 130, 70), (3, 3, 3), (64, 2, 64), (4, 1, 4), 0),       # y: two full chunks, two row segments
    ((99, 5, 9), (3, 3, 33), (3, 1, 3), (66, 2, 1), 6),         # z: chunk 2 sz, the last chunk one plane
    ((131, 6, 9), (3, 3, 3), (4, 1, 4), (64, 3, 1), 0),         # z: three chunks, the last one plane
    ((130, 6, 70), (3, 3, 3), (4, 1, 4), (64, 2, 64), 0),       # z: two full chunks, two row segments
    ((70, 70, 9), (3, 3, 3), (64, 2, 4), (64, 2, 4), 0),        # y and z: two chunks each, the last of four
]
MARCH_IDS = ["y-2sy", "y-three", "y-full", "z-2sz", "z-three", "z-full", "y-and-z"]


def block_labels(seed, shape):
    """Random blocks of LABEL_SET, one to nine voxels along every axis, laid over each other, and
    single voxels on top: nothing lines up with a chunk."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    lab = LABEL_SET[rng.integers(0, len(LABEL_SET), shape)]
    for _ in range(lab.size // 12):
        z, y, x = rng.integers(0, nz), rng.integers(0, ny), rng.integers(0, nx)
        dz, dy, dx = rng.integers(1, 10, 3)
        lab[z:z + dz, y:y + dy, x:x + dx] = LABEL_SET[rng.integers(0, len(LABEL_SET))]
    return np.ascontiguousarray(lab)


def last_chunk(boxes, ym, zm):
    """Which regions (by their box corners) lie in the last chunk of every march that has several."""
    sel = np.ones(len(boxes), bool)
    for corner, (chunk, nch, _) in ((boxes[:, 1], ym), (boxes[:, 2], zm)):
        if nch > 1:
            sel &= corner >= (nch - 1) * chunk
    return sel


def march_case(oracle, shape, size, ym, zm, seed):
    feat, edges, mask, gen = hist_inputs(300 + shape[0], shape)
    lab = block_labels(seed, shape)
    boxes, want = hist_want(oracle, feat, edges, mask, gen, size)
    wants = label_wants(lab, gen, size)
    last = last_chunk(boxes, ym, zm)
    tied = L.dense_ties(lab, gen, size)
    # the per-box oracle on one rule: the last chunk and an even sample of the rest
    some = np.flatnonzero(last | (np.arange(len(boxes)) % max(1, len(boxes) // PER_BOX) == 0))
    per_box = L.roi_labels(lab, boxes[some], *RULES[2])
    frozen(feat, edges, mask, gen, lab, boxes, want, last, tied, some, per_box, *wants.values())
    return dict(feat=feat, edges=edges, mask=mask, gen=gen, size=size, want=want, lab=lab, boxes=boxes,
                wants=wants, last=last, tied=tied, some=some, per_box=per_box)


@pytest.fixture(scope="module", params=MARCHES, ids=MARCH_IDS)
def marched(request, oracle):
    shape, size, ym, zm, seed = request.param
    return request.param, march_case(oracle, shape, size, ym, zm, seed)


def test_marches_cross_what_they_claim(marched):
    (shape, size, ym, zm, _), m = marched
    nz, ny, nx = shape
    assert march(ny, size[1]) == ym and march(nz, size[2]) == zm
    assert ym[1] > 1 or zm[1] > 1
    if shape == (5, 99, 9):
        assert ym[0] == 2 * size[1] > 64
    if shape == (99, 5, 9):
        assert zm[0] == 2 * size[2] > 64
    if nx == 70:
        assert (nx + 63) // 64 == 2 and len(m["boxes"]) > 20000
    # the last chunk holds regions, their histograms are not empty, and the smallest of equal
    # labels is asked for there as well as a unique maximum
    last = m["last"]
    assert 0 < last.sum() < len(last)
    assert m["want"][last].any() and m["want"][~last].any()
    assert m["tied"][last].any() and not m["tied"][last].all()
    assert len(set(m["wants"][RULES[0]][last].tolist())) >= 2
    assert np.array_equal(m["wants"][RULES[2]][m["some"]], m["per_box"])        # the two oracles agree


def test_marches_histograms(ctx, marched):
    _, m = marched
    assert_hist(ctx, m)


def test_marches_labels(ctx, marched):
    _, m = marched
    assert_labels(ctx, m["lab"], m["gen"], m["size"], m["wants"])


# ---- 3. the counters at their last value ---------------------------------------------------------------
# csrc/dense_kernels.hpp: one byte after x (DENSE_MAX_SX = 255), two after y (DENSE_MAX_SXY = 65535).
# volume, box, seed of the labels (one under which each of the two labels wins some region)
LIMITS = [((3, 258, 256), (255, 257, 2), 660), ((2, 21846, 4), (3, 21845, 1), 405)]


@pytest.fixture(scope="module", params=LIMITS, ids=["sx255", "sy21845"])
def limit(request, oracle):
    shape, size, seed = request.param
    nz, ny, nx = shape
    sx, sy, sz = size
    assert sx * sy == 65535 and sx <= 255
    assert (nx - sx + 1, ny - sy + 1, nz - sz + 1) == (2, 2, 2)
    gen = np.zeros(shape, np.uint16)
    gen[sz // 2: sz // 2 + 2, sy // 2: sy // 2 + 2, sx // 2: sx // 2 + 2] = 9       # the eight fitting centres
    gen[0, 0, 0] = gen[-1, -1, -1] = 9                                                # and two whose box does not fit
    feat, edges, mask, _ = hist_inputs(400 + nx, shape)
    boxes, want = hist_want(oracle, feat, edges, mask, gen, size)
    assert len(boxes) == 8
    full = np.ones(shape, np.uint8)
    one_feat = np.empty(shape + (2,), np.float32)
    one_feat[..., 0], one_feat[..., 1] = 1.5, -10.0
    one_edges = np.tile(np.arange(5, dtype=np.float32), (2, 1))                       # 1.5 -> bin 2, -10 -> bin 0
    lab = np.random.default_rng(seed).integers(1, 3, shape).astype(np.uint8)
    wants = label_wants(lab, gen, size)
    assert set(wants[RULES[0]].tolist()) == {1, 2}
    frozen(gen, feat, edges, mask, want, full, one_feat, one_edges, lab, *wants.values())
    return dict(shape=shape, size=size, gen=gen, lab=lab, wants=wants, full=full, one_feat=one_feat,
                one_edges=one_edges, hist=dict(feat=feat, edges=edges, mask=mask, gen=gen, size=size, want=want))


def test_counter_limits_every_voxel_in_one_bin(ctx, limit):
    """The one input that stores 255 after x and 65535 after y."""
    sx, sy, sz = limit["size"]
    got = ctx.dense_roi_histograms(limit["one_feat"], limit["full"], limit["size"], limit["one_edges"],
                                   gen_mask=limit["gen"])
    want = np.zeros((8, 2, 6), np.uint32)
    want[:, 0, 2] = want[:, 1, 0] = sx * sy * sz
    assert sx * sy * sz == (131070 if sx == 255 else 65535)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_counter_limits_random_histograms(ctx, limit):
    assert limit["hist"]["want"].max() > 255
    assert_hist(ctx, limit["hist"])


def test_counter_limits_labels(ctx, limit):
    """Two labels at random: each has about half of the box, so the margin between them is far below
    what a sum cut to 8 or 16 bits loses, and such a cut changes winners."""
    sx, sy, sz = limit["size"]
    votes = np.stack([L._window_sums(limit["lab"] == v, limit["size"]) for v in (1, 2)])
    assert votes.sum(0).min() == sx * sy * sz and np.abs(votes[0] - votes[1]).max() < 2048
    assert_labels(ctx, limit["lab"], limit["gen"], limit["size"], limit["wants"])


def test_dense_roi_labels_refuses_boxes_beyond_the_counters(ctx, ife):
    lib = ife.load_library()
    lab = np.ones((2, 3, 4), np.uint8)
    d = ife._desc(lab.shape, (1.0, 1.0, 1.0))
    out = np.full(8, 77, np.uint8)

    def call(size):
        n = C.c_int64(-1)
        return lib.ife_dense_roi_labels(ctx._h, lab.ctypes.data, ife.U8, lab.ctypes.data, ife.U8, C.byref(d),
                                        ife._size_arg(size), None, 0, -1, out.ctypes.data, len(out), C.byref(n),
                                        ife.MEM_HOST), n.value

    for size in [(3, 21846, 1), (256, 1, 1), (255, 258, 1), (255, 257, 65538)]:
        rc, _ = call(size)
        assert rc == ife.E_SIZE and lib.ife_last_error(ctx._h), size
    assert call((3, 21845, 1)) == (ife.OK, 0) and call((255, 257, 65537)) == (ife.OK, 0)      # too large for the volume only
    assert np.all(out == 77)
    assert np.array_equal(ctx.dense_roi_labels(lab, lab, (3, 3, 1)), np.ones(4, np.uint8))     # still usable


# ---- 4. more work items than one grid -------------------------------------------------------------------
# csrc/dense_capi.inc dense_blocks: a launch has at most 1 << 18 workgroups of four waves, a wave
# takes the work items w, w + 2^20, ...
def test_x_pass_and_label_z_pass_beyond_one_grid(ife):
    """One wave of the x pass per row and one of label_mode_z_kernel per fitting row: 1 050 000 and
    1 049 998.  The rows beyond 2^20 are the second trip of both."""
    shape, size = (1, 1050000, 2), (2, 3, 1)
    nz, ny, nx = shape
    gx, nyv = (nx + 63) // 64, ny - size[1] + 1
    zchunk, nzch, _ = march(nz, size[2])
    wx, wz = gx * ny * nz, gx * nyv * nzch
    assert (wx, wz) == (1050000, 1049998) and wx > GRID_WAVES and wz > GRID_WAVES
    lab = np.random.default_rng(501).integers(0, 3, shape).astype(np.uint8)
    gen = np.ones(shape, np.uint8)
    first = GRID_WAVES - (size[1] - 1)          # regions whose rows all lie in the first trip of the x pass
    with ife.Context(0) as c:
        for rule in RULES[:2]:
            want = L.dense_labels(lab, gen, size, *rule)
            assert want.shape == (wz,) and set(want[first:].tolist()) >= {1, 2}
            got = c.dense_roi_labels(lab, gen, size, *rule)
            assert got.shape == want.shape
            assert np.array_equal(got[:first], want[:first]), (rule, "first trip")
            assert np.array_equal(got[first:GRID_WAVES], want[first:GRID_WAVES]), (rule, "rows of both trips of the x pass")
            assert np.array_equal(got[GRID_WAVES:], want[GRID_WAVES:]), (rule, "second trip")


def test_y_pass_and_histogram_z_pass_beyond_one_grid(ife, oracle):
    """8 components x 255 bins in one group (223 MB of scratch under a bound of 256 MiB): the y pass
    has 2 121 600 work items, the z pass 1 248 480.  The planes of the last components are the
    second trip."""
    shape, size, ncomp, n_edges, scratch_mb = (520, 70, 1), (1, 3, 3), 8, 254, 256
    nz, ny, nx = shape
    nb, nvox = n_edges + 1, nz * ny * nx
    # dense_groups (csrc/dense_capi.inc): whole components while nvox * cg * (1 + 3 nb) fits the budget
    cg = min(ncomp, (scratch_mb << 20) // (nvox * (1 + 3 * nb)), 1024)
    bg = nb
    assert (cg, bg) == (8, 255) and nvox * (3 * cg * bg + cg) < 225e6
    gx, nyv = (nx + 63) // 64, ny - size[1] + 1
    (ychunk, nych, _), (zchunk, nzch, _) = march(ny, size[1]), march(nz, size[2])
    assert (nych, nzch) == (2, 9)
    wy, wz = gx * nz * nych * cg * bg, gx * nyv * nzch * cg * bg
    assert (wy, wz) == (2121600, 1248480) and wy > GRID_WAVES and wz > GRID_WAVES
    feat, _, mask, _ = hist_inputs(502, shape, ncomp, n_edges)
    rng = np.random.default_rng(503)
    edges = np.sort(np.round(rng.normal(0, 3, (ncomp, n_edges)), 2).astype(np.float32), axis=1)
    assert min(len(np.unique(e)) for e in edges) > 200          # most of the 255 bins can be hit
    gen = (rng.random(shape) < 0.01).astype(np.uint16) * 5
    gen[:, ny - 2, 0][::40] = 5                 # centres in the last fitting row
    gen[nz - 2, ::7, 0] = 5                     # and in the last fitting plane
    boxes, want = hist_want(oracle, feat, edges, mask, gen, size)
    assert 300 < len(boxes) < 900
    assert (boxes[:, 1] == ny - 3).any() and (boxes[:, 2] == nz - 3).any()
    # work item = (segment, row or plane, chunk, plane of the counts): the planes from here on are
    # not reached in the first trip
    p_y, p_z = -(-GRID_WAVES // (gx * nz * nych)), -(-GRID_WAVES // (gx * nyv * nzch))
    assert (p_y, p_z) == (1009, 1714) and p_z < cg * bg
    flat = want.reshape(len(boxes), cg * bg)
    assert flat[:, :p_y].any() and flat[:, p_y:p_z].any() and flat[:, p_z:].any()
    with ife.Context(0) as c:
        c.set_option(ife.OPT_DENSE_SCRATCH_MB, scratch_mb)
        got = c.dense_roi_histograms(feat, mask, size, edges, gen_mask=gen)
    assert got.dtype == np.uint32 and got.shape == want.shape
    got = got.reshape(flat.shape)
    assert np.array_equal(got[:, :p_y], flat[:, :p_y]), "first trip of both passes"
    assert np.array_equal(got[:, p_y:p_z], flat[:, p_y:p_z]), "second trip of the y pass"
    assert np.array_equal(got[:, p_z:], flat[:, p_z:]), "second trip of the z pass"
