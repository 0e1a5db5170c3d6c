"""Levels of detail of predicted frames (octree blob version 4), the host side: the plan of a cut
(csrc/octree4_blob.h through GeometryCodec.lod_info) against octree_inter_lod_ref.plan under the encoder's layout and
two layouts no encoder writes, the reference decoder's own check (a plan's prefix decodes, against the reference's
cells alone, to np.unique(points >> k)), the argument checks of decompress(..., reference_lod=), and the plan parser
under the sanitizers (tests/fuzz/fuzz_octree4_lod.cpp, a stand-alone program)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import octree_inter_lod_ref as lod4
import octree_inter_ref as ref4
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "demo-learned-point-cloud-compression_amd", "csrc")
LAYOUTS = {"encoder": None, "S=4": 4, "S=36": 36}


@pytest.fixture(scope="module")
def frames(wl):
    return [f["points"].astype(np.int32) for f in wl.lidar_sequence(3, 16, 300, velocity=(10, 0, 0))]


@pytest.fixture(scope="module")
def blobs(frames):
    """frame 1 coded against frame 0 under every layout; "shallow": the two frames' cells of side 2^9 away from the
    centre of the lattice, a tree of depth 6, so that lod = depth is a level of detail"""
    out = {name: ref4.encode(frames[1], frames[0], S=S) for name, S in LAYOUTS.items()}
    out["shallow"] = ref4.encode(*_shallow(frames)[::-1])
    return out


def _shallow(frames):
    return (frames[0] >> 9) + 100, (frames[1] >> 9) + 100


def _geo_class():
    return pkg("geometry").GeometryCodec


def test_the_frame_is_the_one_the_figures_are_of(frames, blobs):
    h = ref4.header(blobs["encoder"])
    assert (h["n"], sum(h["level_n"]), h["depth"], h["S"], h["nc"]) == (4482, 18808, 16, 148, 2)
    assert len(blobs["encoder"]) == 6216 and h["off_payload"] == 24 + 4 * 16 + 20 + 648 + 4 * 2
    assert [lod4.plan(blobs["encoder"], k)["bytes"] for k in (1, 2, 3, 5, 9, 14, 15)] == [4758, 3240, 2242, 1514, 1168, 1168, 1168]
    assert ref4.header(blobs["S=4"])["nc"] == 74 and ref4.header(blobs["S=36"])["S"] == 36


@pytest.mark.parametrize("layout", list(LAYOUTS) + ["shallow"])
def test_lod_info_is_the_plan(blobs, layout):
    G, abi = _geo_class(), pkg("_abi")
    blob = blobs[layout]
    h = ref4.header(blob)
    depth = h["depth"]
    assert depth == (6 if layout == "shallow" else 16)
    for k in sorted({0, 1, 2, 3, 5, depth - 1, min(depth, 15), 15}):
        pl = lod4.plan(blob, k)
        assert G.lod_info(blob, k) == (pl["bytes"], pl["m"]), k
        assert G.lod_info(blob[:pl["bytes"]], k) == (pl["bytes"], pl["m"]), k      # the same answer from its own prefix
        assert pl["bytes"] <= len(blob) and pl["m"] == (h["n"] if k == 0 else (h["level_n"][depth - k] if k < depth else 1))
        if k == depth - 1:
            assert pl["n_dec"] == 1 and pl["chunks"] == 1 and pl["lanes"] == 1
        if k == 0:
            with pytest.raises(abi.PccError) as e:      # lod 0 stays the whole-blob check
                G.lod_info(blob[:-2], 0)
            assert e.value.code == abi.PCC_E_STREAM
            continue
        # what the plan is computed from: the last needed chunk's length table (N' = 0: the chunk table)
        table_end = pl["bytes"] if pl["n_dec"] == 0 else h["off_payload"] + 2 * (
            sum(np.frombuffer(blob, "<u4", pl["chunks"] - 1, h["off_table"]).tolist()) + 3 * 64)
        assert table_end <= pl["bytes"]
        assert G.lod_info(blob[:table_end], k) == (pl["bytes"], pl["m"]), k
        with pytest.raises(abi.PccError) as e:
            G.lod_info(blob[:table_end - 1], k)
        assert e.value.code == abi.PCC_E_STREAM, k


def test_the_cuts_of_the_forced_layouts_lie_in_later_chunks(blobs):
    assert lod4.plan(blobs["S=4"], 1)["chunks"] == 56 and lod4.plan(blobs["S=4"], 5)["chunks"] >= 2
    assert lod4.plan(blobs["S=36"], 1)["chunks"] == 7 and lod4.plan(blobs["S=36"], 2)["chunks"] >= 2
    assert lod4.plan(blobs["encoder"], 2)["chunks"] == 2 and lod4.plan(blobs["encoder"], 3)["chunks"] == 1


def test_lod_info_refuses_the_other_versions(oracle, frames):
    G, abi = _geo_class(), pkg("_abi")
    with pytest.raises(abi.PccError) as e:
        G.lod_info(oracle.octree_encode(frames[0][:300], 32768, version=1), 1)
    assert e.value.code == abi.PCC_E_ARG
    with pytest.raises(ValueError):
        G.lod_info(b"", 16)


def test_geometry_info_reads_the_head_of_a_prefix(blobs):
    G = _geo_class()
    blob = blobs["encoder"]
    want = G.geometry_info(blob)
    assert want["version"] == 4 and want["predicted"] and want["points"] == 4482
    for k in (1, 2, 5, 15):
        assert G.geometry_info(blob[:G.lod_info(blob, k)[0]]) == want


@pytest.mark.parametrize("layout", list(LAYOUTS) + ["shallow"])
def test_a_plans_prefix_decodes_against_the_references_cells(frames, blobs, layout):
    """the reference decoder's own check, and the claim the feature rests on: the reference's cells are enough"""
    blob = blobs[layout]
    f0, f1 = _shallow(frames) if layout == "shallow" else frames[:2]
    for k in (range(1, 16) if layout in ("encoder", "shallow") else (1, 2, 3, 5, 9, 14, 15)):
        pl = lod4.plan(blob, k)
        got = lod4.decode_lod(blob[:pl["bytes"]], lod4.cells_of(f0, k), k)
        assert np.array_equal(got, lod4.cells_of(f1, k)) and len(got) == pl["m"], k
    with pytest.raises(ValueError):
        lod4.decode_lod(blob[:lod4.plan(blob, 2)["bytes"] - 2], lod4.cells_of(f0, 2), 2)


def test_argument_checks_of_reference_lod():
    """raised before anything touches the device"""
    G = _geo_class()
    geo = G.__new__(G)                # no Runtime: the checks come first
    v2 = bytes([ord("O"), 2]) + bytes(22)
    v4 = ref4.encode(np.array([[1, 2, 3]]), np.array([[1, 2, 3]]))
    ref = np.zeros((1, 3), np.int32)
    with pytest.raises(ValueError, match="frame 1.*version 4.*lod 0"):      # today's refusal, now of the ambiguity
        geo.decompress([v2, v4], lod=2, reference=ref)
    with pytest.raises(ValueError, match="reference_lod"):
        geo.decompress([v2, v4], lod=2, reference=ref)
    for bad in (1, 3, -1, 15, 2.0, True, "2"):
        with pytest.raises(ValueError, match="reference_lod"):
            geo.decompress([v4], lod=2, reference=ref, reference_lod=bad)
    with pytest.raises(ValueError, match="reference_lod"):
        geo.decompress([v4], lod=0, reference=ref, reference_lod=2)
    with pytest.raises(ValueError, match="reference_lod.*without a reference"):
        geo.decompress([v2, v4], lod=2, reference_lod=2)
    with pytest.raises(ValueError, match="lod"):
        geo.decompress([v4], lod=16, reference=ref, reference_lod=16)


def test_octree4_lod_plan_parser_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_octree4_lod")
    src = os.path.join(ROOT, "tests", "fuzz", "fuzz_octree4_lod.cpp")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                            "-w", "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "fuzz:" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
