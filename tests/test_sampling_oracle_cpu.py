"""tests/sampling_oracle.py against the known answers of the sampling definition
(include/ife_hip.h) and against brute force: the admissible voxels listed with np.flatnonzero of
the predicate written out per voxel, indexed by rank."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_oracle as S  # noqa: E402

KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
RANKS = [
    (12345, 0, 1000, [185, 144, 328, 594, 115, 217, 336, 263]),
    (12345, 1, 7, [6, 4, 4, 3, 4, 4, 3, 3]),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % w for w in S.philox4x32_10(counter, key)) == want


@pytest.mark.parametrize("seed,stream,n,want", RANKS)
def test_rank_lists(seed, stream, n, want):
    assert [S.rank(seed, stream, k, n) for k in range(8)] == want


def test_every_rank_is_below_n():
    rng = np.random.default_rng(3)
    for n in [1, 2, 3, 7, 1000, 2 ** 31, 2 ** 32 - 1] + [int(v) for v in rng.integers(1, 2 ** 32, 20)]:
        for k in [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1] + [int(v) for v in rng.integers(0, 2 ** 63, 20)]:
            r = S.rank(int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 32)), k, n)
            assert 0 <= r < n
    assert all(S.rank(9, 9, k, 1) == 0 for k in range(50))


def test_counter_words():
    """k fills the first two counter words, stream + j the third modulo 2^32, the seed the key."""
    k, seed = 5 * 2 ** 32 + 7, 11 * 2 ** 32 + 13
    o = S.philox4x32_10((7, 5, 3, 0), (13, 11))
    assert S.rank(seed, 3, k, 2 ** 32 - 1) == ((o[0] + (o[1] << 32)) * (2 ** 32 - 1)) >> 64
    assert S.rank(seed, 2 ** 32 + 3, k, 1000) == S.rank(seed, 3, k, 1000)
    assert S.rank(seed, 3, k + 2 ** 64, 1000) == S.rank(seed, 3, k, 1000)


@pytest.mark.parametrize("seed,stream,first", [
    (12345, 0, 0),                                 # the draws of RANKS, and a few thousand more
    (6, 9, 2 ** 32 - 3),                           # the draw number crosses into the second counter word
    (6, 9, 2 ** 64 - 3),                           # and wraps at 2^64
    ((0xDEADBEEF << 32) | 6, 2, 5),                # a seed with a high word
    (6, 2 ** 32 - 1, 0), (6, 2 ** 32, 0),          # the last stream, and the one a second set wraps to
])
def test_ranks_equal_rank(seed, stream, first):
    """The vectorised generator against the scalar one, which the known answers above pin."""
    count = 3000 if first == 0 else 40
    numbers = [first + i for i in range(count)]          # Python integers, beyond 2^64 - 1 too
    for n in (1, 7, 1000, 2 ** 31 + 11, 2 ** 32 - 1):
        want = [S.rank(seed, stream, k, n) for k in numbers]
        got = S.ranks(seed, stream, numbers, n)
        assert got.dtype == np.int64 and got.shape == (count,) and [int(v) for v in got] == want
        wrapped = np.array([k % 2 ** 64 for k in numbers], np.uint64)    # and as a uint64 array
        assert np.array_equal(S.ranks(seed, stream, wrapped, n), got)
    assert np.array_equal(S.ranks(seed, stream, np.array(numbers[:12], object).reshape(3, 4), 1000),
                          np.array([S.rank(seed, stream, k, 1000) for k in numbers[:12]]).reshape(3, 4))
    assert S.ranks(seed, stream, [], 5).shape == (0,)


def test_ranks_known_lists_and_the_high_seed_word():
    for seed, stream, n, want in RANKS:
        assert [int(v) for v in S.ranks(seed, stream, range(8), n)] == want
    k = np.arange(64, dtype=np.uint64)
    assert not np.array_equal(S.ranks((0xDEADBEEF << 32) | 6, 0, k, 1000), S.ranks(6, 0, k, 1000))
    assert np.array_equal(S.ranks(6, 2 ** 32 + 3, k, 1000), S.ranks(6, 3, k, 1000))


def _brute_fits(shape, size):
    nz, ny, nx = shape
    out = np.zeros(shape, bool)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                lo = (x - size[0] // 2, y - size[1] // 2, z - size[2] // 2)
                out[z, y, x] = all(l >= 0 and l + s <= n for l, s, n in zip(lo, size, (nx, ny, nz)))
    return out


@pytest.mark.parametrize("size", [(1, 1, 1), (2, 2, 2), (5, 4, 3), (9, 7, 5), (10, 1, 1), (1, 8, 6)])
def test_fits_equals_brute_force(size):
    shape = (5, 7, 9)
    assert np.array_equal(S.fits(shape, size), _brute_fits(shape, size))
    if size[0] > 9:
        assert not S.fits(shape, size).any()


@pytest.mark.parametrize("size", [(1, 1, 1), (5, 4, 3), (4, 2, 2)])
@pytest.mark.parametrize("values,per_value", [((), False), ((1, 3), False), ((3, 1, 3, 200), True)])
def test_draws_equal_brute_force(size, values, per_value):
    rng = np.random.default_rng(5)
    mask = rng.integers(0, 5, (5, 7, 9)).astype(np.uint8)
    f = _brute_fits(mask.shape, size)
    if not values:
        preds = [np.array([v != 0 for v in mask.ravel()])]
    elif not per_value:
        preds = [np.array([v in values for v in mask.ravel()])]
    else:
        preds = [np.array([v == w for v in mask.ravel()]) for w in values]
    lists = [np.flatnonzero(p & f.ravel()) for p in preds]
    got = S.admissible(mask, size, values, per_value)
    assert len(got) == len(lists) and all(np.array_equal(a, b) for a, b in zip(got, lists))
    if any(len(a) == 0 for a in lists):
        with pytest.raises(ValueError):
            S.sample_positions(mask, 4, size, values, per_value, seed=1)
        pos, counts = S.sample_positions(mask, 0, size, values, per_value, seed=1)
        assert pos.shape == (len(lists), 0) and list(counts) == [len(a) for a in lists]
        return
    pos, counts = S.sample_positions(mask, 40, size, values, per_value, seed=77, stream=2, first_draw=5)
    assert list(counts) == [len(a) for a in lists]
    for j, a in enumerate(lists):
        assert [int(v) for v in pos[j]] == [int(a[S.rank(77, 2 + j, 5 + i, len(a))]) for i in range(40)]
    boxes = S.boxes_of(pos, mask.shape, size)
    nz, ny, nx = mask.shape
    assert (boxes[..., :3] >= 0).all() and (boxes[..., 0] + size[0] <= nx).all()
    assert (boxes[..., 1] + size[1] <= ny).all() and (boxes[..., 2] + size[2] <= nz).all()
    assert np.array_equal(boxes[..., 0] + size[0] // 2 + nx * (boxes[..., 1] + size[1] // 2 + ny * (boxes[..., 2] + size[2] // 2)), pos)


def test_extract_and_lines():
    src = np.arange(5 * 7 * 9, dtype=np.float32).reshape(5, 7, 9)
    out = S.extract_rois(src, [[1, 2, 0, 3, 2, 4], [6, 5, 1, 3, 2, 4]])
    assert out.shape == (2, 4, 2, 3) and out[1, 3, 1, 2] == src[4, 6, 8]
    assert S.roi_info_lines([[1, 2, 0, 3, 2, 4]]) == ["[1, 2, 0][3, 2, 4]"]
