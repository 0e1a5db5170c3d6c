"""The z job of the whole-GOP decoder reads the z string through coder tables the codec built once
(pcc_rans_decode8_gated with prebuilt tables, byte indexes, no chunk gate: csrc/rans_host.cpp).  That path under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, beside tests/test_fuzz_host.py: intact, damaged and cut
streams give the generic decoder's symbols or its error, never a report."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "demo-learned-point-cloud-compression_amd", "csrc")


def test_cached_table_decoder_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_rans_tables")
    src = os.path.join(ROOT, "tests", "fuzz", "fuzz_rans_tables.cpp")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-pthread",
                            "-w", "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "cached tables equal generic: 1" in run.stdout and "0 differ from the generic decoder" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
