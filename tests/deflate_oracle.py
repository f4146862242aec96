"""The block format of ife_deflate (include/ife_hip.h), restated in plain Python for the tests.

Input of n bytes in chunks of C = 32768.  Every chunk becomes complete, non-final DEFLATE blocks
that start and end on a byte boundary; the chunks' byte strings are concatenated.

Tokens of a chunk [lo, hi): eq[i] holds when i >= 4 and b[i] == b[i-4] (global index).  Where eq
is false the byte is a literal.  A maximal run [i, j) of true eq inside the chunk (a run running at
lo starts at lo) of length L >= 3 becomes matches of distance 4 and length min(258, rest) while
rest >= 3, the 0, 1 or 2 bytes left over are literals; a run shorter than 3 is literals.

Form F: a fixed-Huffman block (BFINAL 0, BTYPE 01), the tokens, end of block, then an empty stored
block (three zero bits, padding to the byte, 00 00 FF FF).  Form S: one stored block, 5 + len
bytes.  The chunk takes S when S is not longer than F.
"""
import numpy as np

C = 32768


def bound(n):
    return n + 5 * ((n + C - 1) // C)


def _rev(code, nbits):
    r = 0
    for _ in range(nbits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def _fixed_code(sym):
    """(code, bits) of a literal/length symbol in the fixed tree of RFC 1951, 3.2.6."""
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + (sym - 144), 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + (sym - 280), 8


_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99,
             115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)

# what goes into the bit stream, LSB first: (value, bits)
_LIT = []
for _v in range(256):
    _c, _n = _fixed_code(_v)
    _LIT.append((_rev(_c, _n), _n))
_EOB = (_rev(*_fixed_code(256)), 7)
_DIST4 = (_rev(3, 5), 5)  # distance 4 is distance code 3, no extra bits


def _match(length):
    k = max(i for i in range(29) if _LEN_BASE[i] <= length)
    if length == 258:
        k = 28
    c, n = _fixed_code(257 + k)
    val, bits = _rev(c, n), n
    val |= (length - _LEN_BASE[k]) << bits
    bits += _LEN_EXTRA[k]
    val |= _DIST4[0] << bits
    return val, bits + 5


_MATCH = [None, None, None] + [_match(L) for L in range(3, 259)]


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, val, bits):
        self.acc |= val << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.out.append(self.acc & 0xFF)
            self.acc = 0
            self.n = 0


def tokens(b, eq, lo, hi):
    """The tokens of chunk [lo, hi): ('L', byte) and ('M', length)."""
    out = []
    i = lo
    while i < hi:
        if not eq[i]:
            out.append(("L", int(b[i])))
            i += 1
            continue
        j = i
        while j < hi and eq[j]:
            j += 1
        rest = j - i
        if rest >= 3:
            while rest >= 3:
                m = min(258, rest)
                out.append(("M", m))
                rest -= m
        for k in range(j - rest, j):
            out.append(("L", int(b[k])))
        i = j
    return out


def fixed_blocks(b, eq, lo, hi):
    """Form F of chunk [lo, hi)."""
    w = _Bits()
    w.put(0, 1)   # BFINAL
    w.put(1, 2)   # BTYPE 01
    for kind, v in tokens(b, eq, lo, hi):
        w.put(*(_LIT[v] if kind == "L" else _MATCH[v]))
    w.put(*_EOB)
    w.put(0, 3)   # an empty stored block realigns
    w.align()
    return bytes(w.out) + b"\x00\x00\xff\xff"


def chunk_blocks(b, eq, lo, hi):
    f = fixed_blocks(b, eq, lo, hi)
    n = hi - lo
    if 5 + n <= len(f):
        return b"\x00" + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + bytes(b[lo:hi])
    return f


def deflate_blocks(data):
    """The blocks of `data` (bytes-like): append 03 00 and it is a raw DEFLATE stream."""
    b = np.frombuffer(bytes(data), np.uint8)
    n = b.size
    eq = np.zeros(n, bool)
    if n > 4:
        eq[4:] = b[4:] == b[:-4]
    return b"".join(chunk_blocks(b, eq, lo, min(lo + C, n)) for lo in range(0, n, C))


def inflate(blocks):
    import zlib
    d = zlib.decompressobj(-15)
    out = d.decompress(bytes(blocks) + b"\x03\x00")
    assert d.eof and not d.unused_data
    return out


# ---- the inputs both test files use ---------------------------------------------------------
SIZES = (0, 1, 3, 4, 5, 7, 262, C - 1, C, C + 1, 2 * C + 7, 3 * C + 1)
RUN_LENGTHS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 518, 519, 520)


def run_offsets(L):
    return (10, C - L // 2 - 2, C - 1, C, C + 1)


def planted_run(L, at, seed=0):
    """2C + 64 random bytes with one run of exactly L bytes that repeat the four before them,
    beginning at `at`.  Chunk 0 is zero up to C - 3000 and chunk 1 from C + 3000 on, but for the
    surroundings of the run and one stretch with all 256 byte values, so form F wins in both and
    every literal code occurs."""
    return planted_runs(L, (at,), seed)


def planted_runs(L, ats, seed=0):
    """planted_run with one run of exactly L bytes at every offset of `ats` (ascending, at least
    600 bytes from the end of one run to the start of the next, none over the stretch of all byte
    values): the same background, and every run is exactly [at, at + L)."""
    ats = tuple(ats)
    rng = np.random.default_rng(1000 * L + ats[0] + seed)
    b = rng.integers(0, 256, 2 * C + 64, dtype=np.uint8)
    for prev, at in zip(ats, ats[1:]):
        assert at - (prev + L) >= 600, (L, prev, at)
    for at in ats:
        assert at >= 5 and at + L + 8 <= b.size and (at + L + 8 <= 4096 or at - 8 >= 4096 + 256), (L, at)
    keep = [b[max(0, at - 8):at + L + 8].copy() for at in ats]
    b[:C - 3000] = 0
    b[C + 3000:2 * C] = 0
    b[4096:4096 + 256] = np.arange(256, dtype=np.uint8)
    for at, k in zip(ats, keep):
        b[max(0, at - 8):at + L + 8] = k
    for at in ats:
        for i in range(at, at + L):
            b[i] = b[i - 4]
        for i in (at - 1, at + L):  # the run is exactly [at, at + L)
            if b[i] == b[i - 4]:
                b[i] ^= 0x55
        eq = b[at - 1:at + L + 1] == b[at - 5:at + L - 3]
        assert not eq[0] and eq[1:-1].all() and not eq[-1]
    return b.tobytes()


# Thread t of a chunk's workgroup owns bytes [128t, 128t + 128), a wave 8192: where the device hands
# the start and the end of a run from one thread, and one wave, to the next.
SEAM_LENGTHS = (1, 2, 3, 4, 127, 128, 129, 257, 258, 259, 260, 261, 516, 519)
SEAM_STARTS = (8191, 9472, 10753)          # 127, 0, 1 modulo 128; the first at a wave seam
# Exclusive ends, 0, 127, 1 modulo 128.  The first and the last are at wave seams, where the last
# block of the run begins in one wave and takes its length from a break in the next.
SEAM_ENDS = (16384, 17791, 24577)


def seam_offsets(L):
    """Six starts of runs of L bytes in chunk 0: three begin and three end (exclusive) one byte
    before, at and one byte behind a thread seam, at least one of each at a wave seam."""
    ats = SEAM_STARTS + tuple(e - L for e in SEAM_ENDS)
    assert sorted(a % 128 for a in ats[:3]) == [0, 1, 127]
    assert sorted((a + L) % 128 for a in ats[3:]) == [0, 1, 127]
    assert any(abs(a - 8192 * round(a / 8192)) <= 1 for a in ats[:3])
    assert any(abs(a + L - 8192 * round((a + L) / 8192)) <= 1 for a in ats[3:])
    assert ats[-1] + L + 8 < C - 3000  # all in chunk 0, inside its zeros
    return ats


def seam_cases():
    """name -> bytes, one buffer per length of SEAM_LENGTHS with the six runs of seam_offsets."""
    return {"seams_%d" % L: planted_runs(L, seam_offsets(L)) for L in SEAM_LENGTHS}


def _no_eq_bytes(rng, n):
    """n bytes under 144 (literals of 8 bits), none equal to the byte four before it."""
    b = rng.integers(0, 144, n, dtype=np.uint8)
    for i in range(4, n):
        while b[i] == b[i - 4]:
            b[i] = rng.integers(0, 144)
    return b


def _plant_exact(b, at, L):
    """Makes [at, at + L) the only run of b, which had none; the bytes stay under 144."""
    for i in range(at, at + L):
        b[i] = b[i - 4]
    for i in range(at + L, b.size):  # a changed byte may equal the one four behind it
        if b[i] == b[i - 4]:
            b[i] = (b[i] + 1) % 144
    eq = np.zeros(b.size, bool)
    eq[4:] = b[4:] == b[:-4]
    assert eq[at:at + L].all() and eq.sum() == L and b.max() < 144


TIE_RUNS = (0, 3, 4)  # no run: S by one byte; a run of 3: the tie, S; a run of 4: F by one byte


def tie_cases():
    """name -> bytes.  For n in (1000, C) and a run of r in TIE_RUNS bytes: literals of 8 bits
    only, so form F takes n + 6, n + 5 (as long as S) and n + 4 bytes.  The run begins on the last
    byte of a thread (128k + 127).  tie_<C + 1000>_3 has the tie in chunk 0 and a stored chunk
    behind it, which a wrong size of chunk 0 misplaces."""
    cases = {}
    for n, at, total in ((1000, 383, 1000), (C, 128 * 100 + 127, C), (C, 128 * 100 + 127, C + 1000)):
        for r in TIE_RUNS:
            if total != n and r != 3:
                continue
            b = _no_eq_bytes(np.random.default_rng(7000 + total + r), total)
            if r:
                _plant_exact(b, at, r)
            eq = np.zeros(total, bool)
            eq[4:] = b[4:] == b[:-4]
            flen = len(fixed_blocks(b, eq, 0, n))
            got = chunk_blocks(b, eq, 0, n)
            assert flen == {0: n + 6, 3: n + 5, 4: n + 4}[r], (n, r, flen)
            assert (got[0] == 0 and len(got) == n + 5) if r < 4 else (got[0] != 0 and len(got) == n + 4)
            cases["tie_%d_%d" % (total, r)] = b.tobytes()
    return cases


def edge_counts(mis):
    """The two lengths at which, for a source `mis` bytes behind a 16-byte boundary, thread 0's
    bytes end with its eighth 16-byte granule and reach one byte into the ninth."""
    assert 0 <= mis < 16
    return (128 - mis, 129 - mis)


def edge_case(n):
    """n zero bytes with random non-zero bytes at fixed places, the last byte among them, so that
    matches and literals both occur and a last byte that was not loaded shows."""
    b = np.zeros(n, np.uint8)
    at = [i for i in (0, 5, 6, 7, 40, 77, 78, n - 17, n - 2, n - 1) if 0 <= i < n]
    b[at] = np.random.default_rng(n).integers(1, 256, len(at), dtype=np.uint8)
    return b.tobytes()


def masked_volume(shape=(20, 24, 40), seed=5):
    """float32 values inside an ellipsoid, exact zeros outside."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij")
    inside = (z / 0.8) ** 2 + (y / 0.7) ** 2 + (x / 0.6) ** 2 < 1.0
    v = rng.standard_normal(shape).astype(np.float32)
    return np.where(inside, v, np.float32(0)).astype(np.float32)


def crossing_runs():
    """Three chunks; the run that crosses each chunk start began in the chunk before: zeros over
    the first boundary, a repeated four-byte pattern over the second."""
    rng = np.random.default_rng(11)
    b = np.zeros(3 * C, np.uint8)
    for c in range(3):
        b[c * C + 9000:c * C + 14000] = rng.integers(0, 256, 5000, dtype=np.uint8)
    b[2 * C - 1003:2 * C + 777] = np.resize(np.array([1, 2, 3, 250], np.uint8), 1780)
    return b.tobytes()


def small_cases():
    """name -> bytes: every input that is compared with the restatement byte for byte."""
    cases = {}
    rng = np.random.default_rng(3)
    for n in SIZES:
        cases["zeros_%d" % n] = bytes(n)
        cases["random_%d" % n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    cases["ones_f32"] = np.ones(20000, np.float32).tobytes()
    for L in RUN_LENGTHS:
        for at in run_offsets(L):
            cases["run_%d_at_%d" % (L, at)] = planted_run(L, at)
    cases["masked_volume"] = masked_volume().tobytes()
    cases["crossing_runs"] = crossing_runs()
    cases.update(tie_cases())
    cases.update(seam_cases())
    for n in sorted({n for mis in range(16) for n in edge_counts(mis)}):
        cases["edge_%d" % n] = edge_case(n)
    return cases
