"""The parsers of the near-lossless attribute blobs, versions 4 and 7 (csrc/attr_blob.h attr_parse_kind /
attr2_parse_kind), which read untrusted bytes and prefixes before anything is reserved or launched, under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: damaged and cut blobs at random levels of detail give error
codes, max_error is held to the value width, an accepted plan sizes nothing beyond the bytes present, the lossless kinds
parse as before, and no sanitizer reports."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "demo-learned-point-cloud-compression_amd", "csrc")


def test_attr_nl_parsers_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_attr_nl_header")
    src = os.path.join(ROOT, "tests", "fuzz", "fuzz_attr_nl_header.cpp")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                            "-w", "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert "fuzz:" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
