"""The block plan of the dense bag stream (csrc/dense_plan.hpp) is plain host code: a stand-alone
program (tests/csrc/dense_plan_main.cpp, its own main) is built with the address and
undefined-behaviour sanitizers and run.  Its cases: one block for everything, a bound of one row
(one plane per block), a plane count the block size does not divide, empty planes at the start,
in the middle and at the end, zero regions; rows covered exactly once in each."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-feature-extraction_amd", "csrc")


def test_dense_plan_sanitized(tmp_path):
    exe = str(tmp_path / "dense_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "csrc", "dense_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dense plan ok" in r.stdout and "FAIL" not in r.stdout
    for case in ("one block", "bound of one row", "plane count not divided", "empty planes", "zero regions"):
        assert case + ":" in r.stdout, case


def test_dense_plan_has_no_hip_include():
    txt = open(os.path.join(CSRC, "dense_plan.hpp")).read()
    assert "hip/" not in txt and "hip_runtime" not in txt
