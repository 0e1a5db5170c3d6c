"""The parser of the transform-coded attribute blob with level-of-detail prefixes, version 22 (csrc/attr_blob.h
attr_s_parse and the plan it shares with version 2, attr_lod_plan), which reads untrusted bytes and prefixes before
anything is reserved or launched, under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: well-formed heads are
accepted and read back at every level 0 .. K, from the plan's bytes and not from one byte less; a K of 0 or beyond 15 -
slod, counts that are not version 2's, and a level above K are refused; byte 22 is refused by the ten other parsers and
their bytes by this one, and no sanitizer reports.  Host code only, in a program of its own."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "demo-learned-point-cloud-compression_amd", "csrc")


def test_attr_scalable_parser_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_attr_scalable_header")
    src = os.path.join(ROOT, "tests", "fuzz", "fuzz_attr_scalable_header.cpp")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                            "-w", "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert "fuzz:" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
