"""The block format of ife_deflate without a GPU.

The Python restatement (tests/deflate_oracle.py) inflates to its input through zlib and keeps the
bound.  Two stand-alone programs (their own main, built with the address and undefined-behaviour
sanitizers) run the plain C++ of the product: the token walk, bit packing and CRC arithmetic of
csrc/deflate_kernels.hpp driven thread by thread as the kernel drives them, which must give the
restatement's bytes, and the gzip assembler of the host mirror (ife/Host/ImageIO.h), whose file
Python's gzip module must accept (it checks CRC and length) and decode to header plus payload."""
import gzip
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_oracle as dfo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-feature-extraction_amd")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]
C = dfo.C


@pytest.fixture(scope="module")
def cases():
    return {k: (v, dfo.deflate_blocks(v)) for k, v in dfo.small_cases().items()}


def test_restatement_inflates_and_keeps_the_bound(cases):
    for name, (data, blocks) in cases.items():
        assert dfo.inflate(blocks) == data, name
        assert len(blocks) <= dfo.bound(len(data)), name
        if name.startswith("random_"):
            assert len(blocks) == dfo.bound(len(data)), name  # stored
    assert dfo.deflate_blocks(b"") == b"" and dfo.bound(0) == 0
    assert dfo.bound(1) == 6 and dfo.bound(C) == C + 5 and dfo.bound(C + 1) == C + 11
    for size in (C - 1, C, C + 1, 3 * C + 1):  # zeros: one match per 258 bytes, 13 bits each
        assert len(dfo.deflate_blocks(bytes(size))) < size // 100


def test_tokens_of_the_run_lengths():
    """What the format says of runs: 258, 258 + 1 literal, 258 + 2 literals, 258 + 3."""
    for L, want in ((1, ["L"]), (2, ["L", "L"]), (3, [3]), (4, [4]), (257, [257]), (258, [258]),
                    (259, [258, "L"]), (260, [258, "L", "L"]), (261, [258, 3]), (516, [258, 258]),
                    (517, [258, 258, "L"]), (518, [258, 258, "L", "L"]), (519, [258, 258, 3]),
                    (520, [258, 258, 4])):
        b = np.frombuffer(dfo.planted_run(L, 100), np.uint8)
        eq = np.zeros(b.size, bool)
        eq[4:] = b[4:] == b[:-4]
        toks = dfo.tokens(b, eq, 100, 100 + L)
        assert [t[1] if t[0] == "M" else "L" for t in toks] == want, L


def test_kernel_walk_on_the_host_equals_the_restatement(cases, tmp_path):
    exe = str(tmp_path / "deflate_walk_main")
    subprocess.check_call(SAN + ["-I", os.path.join(PKG, "csrc"),
                                 os.path.join(ROOT, "tests", "csrc", "deflate_walk_main.cpp"), "-o", exe])
    for k, (name, (data, blocks)) in enumerate(cases.items()):
        (tmp_path / "in.bin").write_bytes(data)
        # every alignment of the chunk image in turn
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(k % 16)],
                           capture_output=True, text=True)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        assert (tmp_path / "out.bin").read_bytes() == blocks, name
        assert int(r.stdout.split()[1], 16) == zlib.crc32(data), name


def test_kernel_header_core_has_no_hip_outside_its_guard():
    txt = open(os.path.join(PKG, "csrc", "deflate_kernels.hpp")).read()
    plain = txt.split("#ifdef __HIPCC__\n\n__device__", 1)[0]
    assert "threadIdx" not in plain and "__shared__" not in plain and "__global__" not in plain


def test_gzip_assembler_sanitized(cases, tmp_path):
    exe = str(tmp_path / "gzip_member_main")
    subprocess.check_call(SAN + ["-I", os.path.join(PKG, "host", "include"), "-I", os.path.join(ROOT, "include"),
                                 os.path.join(ROOT, "tests", "csrc", "gzip_member_main.cpp"), "-o", exe, "-lz"])
    head = bytes(range(256)) + bytes(96)  # 352 bytes, as the NIfTI header and its extension
    (tmp_path / "head.bin").write_bytes(head)
    for name in ("masked_volume", "zeros_0", "random_%d" % (C + 1), "crossing_runs", "run_259_at_%d" % (C - 1)):
        data, blocks = cases[name]
        (tmp_path / "blocks.bin").write_bytes(blocks)
        out = tmp_path / (name + ".gz")
        r = subprocess.run([exe, str(tmp_path / "head.bin"), str(tmp_path / "blocks.bin"),
                            "%08x" % zlib.crc32(data), str(len(data)), str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and "gzip member ok" in r.stdout, name + ": " + r.stdout + r.stderr
        raw = out.read_bytes()
        assert raw[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])
        assert gzip.decompress(raw) == head + data, name
        with gzip.open(str(out), "rb") as f:  # the file interface reads the trailer too
            assert f.read() == head + data
    # a wrong CRC must not pass: the check above is the reader's, not ours
    data, blocks = cases["masked_volume"]
    (tmp_path / "blocks.bin").write_bytes(blocks)
    subprocess.check_call([exe, str(tmp_path / "head.bin"), str(tmp_path / "blocks.bin"),
                           "%08x" % (zlib.crc32(data) ^ 1), str(len(data)), str(tmp_path / "bad.gz")],
                          stdout=subprocess.DEVNULL)
    with pytest.raises(gzip.BadGzipFile):
        gzip.decompress((tmp_path / "bad.gz").read_bytes())
