"""Predicted frames (octree blob version 4) at a level of detail on the GPU (csrc/octree4.hip,
pcc_octree_decode_frames_refs_lod, GeometryCodec.decompress(..., lod=k, reference_lod=)): a prefix of a predicted blob,
decoded against the CELLS of the frames in front of it, gives byte for byte np.unique(frame >> k) in Morton order and
what version 2's prefix of the same frame gives — for chains, blobs under layouts no encoder writes (each asserting from
the header the property it is there for), streaming receivers that hold cells or lattice points, history windows,
intra_period mixes, frames without points, root cubes that differ, attributes beside the geometry and the other
output forms.  A wrong reference and a damaged word above the cut follow the documented contract: PccError, or m
rows; the call after them decodes."""
import struct

import numpy as np
import pytest

import octree_inter_lod_ref as lod4
import octree_inter_ref as ref4
from conftest import pkg, random_cloud

pytestmark = pytest.mark.gpu
SEQ = dict(n_frames=5, rings=16, azimuths=300, velocity=(10, 0, 0))


@pytest.fixture(scope="module")
def geo(rt):
    g = pkg().GeometryCodec()
    yield g
    g.close()


@pytest.fixture(scope="module")
def frames(wl):
    """five sweeps; the first three are the sequence the CPU tests of the plan use"""
    return [f["points"].astype(np.int32) for f in wl.lidar_sequence(SEQ["n_frames"], SEQ["rings"], SEQ["azimuths"], velocity=SEQ["velocity"])]


def _cells(p, k):
    return lod4.cells_of(p, k).astype(np.int32).reshape(-1, 3) if len(p) else np.zeros((0, 3), np.int32)


def _cut(blob, k, more=0):
    return blob[:pkg().GeometryCodec.lod_info(blob, k)[0] + more]


def _same(got, frames, k, v2=None):
    assert len(got) == len(frames)
    for f, (g, p) in enumerate(zip(got, frames)):
        assert g.dtype == np.int32 and g.shape == (len(_cells(p, k)), 3) and np.array_equal(g, _cells(p, k)), (f, k)
        if v2 is not None:
            assert np.array_equal(g, v2[f]), (f, k)


def _v2_cells(geo, frames, k):
    return geo.decompress([_cut(b, k) for b in geo.compress(frames)], lod=k)


def _refused(geo, abi, blobs, k, **kw):
    with pytest.raises(abi.PccError) as e:
        geo.decompress(blobs, lod=k, **kw)
    return e.value


# ------------------------------------------------------------------ the chain I P P
@pytest.mark.parametrize("k", [1, 2, 3, 5, 15])
def test_chain_of_the_encoders_blobs(geo, frames, k):
    """depth 16: k = 15 is depth - 1, one node above the cut"""
    abi, chain = pkg("_abi"), frames[:3]
    blobs = geo.compress(chain, predict="previous")
    assert [b[1] for b in blobs] == [2, 4, 4] and all(b[2] == 16 for b in blobs)
    v2 = _v2_cells(geo, chain, k)
    _same(geo.decompress(blobs, lod=k), chain, k, v2)                      # whole blobs
    for more in (0, 1, 7):                                                 # the prefixes lod_info names, and longer ones
        _same(geo.decompress([_cut(b, k, more) for b in blobs], lod=k), chain, k, v2)
    short = [_cut(blobs[0], k), _cut(blobs[1], k), _cut(blobs[2], k, -2)]
    err = _refused(geo, abi, short, k)                                     # on the host, before anything is launched
    assert err.code == abi.PCC_E_STREAM and "frame 2" in str(err) and "truncated" in str(err)
    _same(geo.decompress([_cut(b, k) for b in blobs], lod=k), chain, k, v2)


@pytest.mark.parametrize("k", ["depth - 1", "depth", 15])
def test_chain_of_a_shallow_tree(geo, frames, k):
    """cells of side 2^9 away from the lattice's centre: depth 6, so that k = depth and k > depth exist (nothing is
    decoded, the one cell is the root cube's)"""
    abi, chain = pkg("_abi"), [(f >> 9) + 100 for f in frames[:3]]
    blobs = geo.compress(chain, predict="previous")
    depth = blobs[1][2]
    assert [b[1] for b in blobs] == [2, 4, 4] and depth == 6
    k = {"depth - 1": depth - 1, "depth": depth}.get(k, k)
    v2 = _v2_cells(geo, chain, k)
    _same(geo.decompress(blobs, lod=k), chain, k, v2)
    for more in (0, 1, 7):
        _same(geo.decompress([_cut(b, k, more) for b in blobs], lod=k), chain, k, v2)
    err = _refused(geo, abi, [_cut(blobs[0], k), _cut(blobs[1], k, -2)], k)
    assert err.code == abi.PCC_E_STREAM and "frame 1" in str(err)
    _same(geo.decompress([_cut(b, k) for b in blobs], lod=k), chain, k, v2)


# ------------------------------------------------------------------ blobs the encoder never writes
# found on the CPU with octree_inter_ref.build_tree over _boundary_cloud(seed), seeds 0, 1, 2, ..: the first cloud with a
# level that begins at a multiple of 256 nodes, a chunk boundary under S = 4
CHUNK_BOUNDARY_SEED = 18


def _boundary_cloud(seed):
    rng = np.random.default_rng(seed)
    return np.unique(rng.integers(-150, 150, (400, 3)), axis=0).astype(np.int32)


@pytest.fixture(scope="module")
def forced(frames):
    """name -> (frame, reference, blob of the reference coder under a forced S), coded once when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            frame, reference, S = {
                "S=4, many chunks": (np.concatenate([frames[1], frames[2]]), frames[0], 4),
                "S=36": (frames[1], frames[0], 36),
                "S=4, boundaries": (_boundary_cloud(CHUNK_BOUNDARY_SEED), _boundary_cloud(CHUNK_BOUNDARY_SEED + 100), 4),
            }[name]
            made[name] = (frame, reference, ref4.encode(frame, reference, S=S))
        return made[name]
    return get


def _forced_case(geo, forced, name, k):
    """the cut's plan; the prefix decoded against the reference's cells, checked"""
    frame, reference, blob = forced(name)
    pl = lod4.plan(blob, k)
    assert geo.lod_info(blob, k) == (pl["bytes"], pl["m"])
    want = _cells(frame, k)
    (v2,) = _v2_cells(geo, [frame], k)
    for piece in (blob, blob[:pl["bytes"]], blob[:pl["bytes"] + 1]):
        (got,) = geo.decompress([piece], lod=k, reference=_cells(reference, k), reference_lod=k)
        assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(got, v2), (name, k, len(piece))
    return pl, ref4.header(blob)


def test_a_cut_above_64_chunks(geo, forced):
    """the wave that decodes chunk c sums c entries of the chunk table, 64 at a time"""
    pl, h = _forced_case(geo, forced, "S=4, many chunks", 1)
    assert h["S"] == 4 and pl["chunks"] > 64 and h["nc"] > pl["chunks"]


def test_a_layout_of_36_nodes_per_lane(geo, forced):
    pl, h = _forced_case(geo, forced, "S=36", 2)
    assert h["S"] == 36 and 1 < pl["chunks"] < h["nc"]


def test_a_cut_in_the_middle_of_a_lanes_run(geo, forced):
    """the last lane stops two nodes into its run of four and leaves a carry that nothing picks up"""
    pl, h = _forced_case(geo, forced, "S=4, boundaries", 3)
    assert h["S"] == 4 and pl["n_dec"] % 4 == 2


def test_a_cut_on_a_lane_boundary(geo, forced):
    """N' is a multiple of S and not of 64 S: the last needed lane ends with the cut, all its words consumed"""
    pl, h = _forced_case(geo, forced, "S=4, boundaries", 2)
    assert pl["n_dec"] % h["S"] == 0 and pl["n_dec"] % (64 * h["S"]) != 0


def test_a_cut_on_a_chunk_boundary(geo, forced):
    """N' is a multiple of 64 S: the last needed chunk is needed whole and the next one not at all"""
    pl, h = _forced_case(geo, forced, "S=4, boundaries", 5)
    assert pl["n_dec"] == 256 == 64 * h["S"] and pl["chunks"] == 1 and pl["lanes"] == 64 and h["nc"] > 1


# ------------------------------------------------------------------ streaming: one blob per call
@pytest.mark.parametrize("k", [2, 5])
def test_streaming_receivers(geo, frames, k):
    import torch
    chain = frames[:3]
    blobs = [_cut(b, k) for b in geo.compress(chain, predict="previous")]
    (held,) = geo.decompress(blobs[:1], lod=k)                       # a receiver that never held full resolution
    for f in (1, 2):
        (cells,) = geo.decompress([blobs[f]], lod=k, reference=held, reference_lod=k)
        assert np.array_equal(cells, _cells(chain[f], k)), f
        (from_points,) = geo.decompress([blobs[f]], lod=k, reference=chain[f - 1], reference_lod=0)
        assert np.array_equal(from_points, cells), f
        held = cells
    # the same from device tensors, and from rows in another order with repeats
    dev = torch.from_numpy(_cells(chain[1], k)).to(geo.rt.device)
    (cells,) = geo.decompress([blobs[2]], lod=k, reference=dev, reference_lod=k, output="device")
    assert np.array_equal(cells.cpu().numpy(), _cells(chain[2], k))
    shuffled = np.concatenate([_cells(chain[1], k), _cells(chain[1], k)[:9]])[::-1].copy()
    assert np.array_equal(geo.decompress([blobs[2]], lod=k, reference=shuffled, reference_lod=k)[0], _cells(chain[2], k))


# ------------------------------------------------------------------ history and mixes
def test_history_windows(geo, frames):
    """history=3 over five frames: windows of 1, 2, 3, 3 frames, the unions formed from the cells' keys"""
    G, k = pkg().GeometryCodec, 2
    blobs = geo.compress(frames, predict="previous", history=3)
    assert [G.reference_frames(b) for b in blobs] == [0, 1, 2, 3, 3]
    v2 = _v2_cells(geo, frames, k)
    _same(geo.decompress(blobs, lod=k), frames, k, v2)
    cut = [_cut(b, k) for b in blobs]
    _same(geo.decompress(cut, lod=k), frames, k, v2)
    held = [_cells(f, k) for f in frames[1:4]]                       # the last three decoded frames, oldest first
    assert np.array_equal(geo.decompress([cut[4]], lod=k, reference=held, reference_lod=k)[0], _cells(frames[4], k))
    assert np.array_equal(geo.decompress([cut[4]], lod=k, reference=frames[1:4], reference_lod=0)[0], _cells(frames[4], k))
    _same(geo.decompress(cut[3:], lod=k, reference=[_cells(f, k) for f in frames[:3]], reference_lod=k), frames[3:], k)


def test_intra_period_mixes_the_versions(geo, frames):
    k = 3
    blobs = geo.compress(frames, predict="previous", intra_period=2)
    assert [b[1] for b in blobs] == [2, 4, 2, 4, 2]
    _same(geo.decompress([_cut(b, k) for b in blobs], lod=k), frames, k, _v2_cells(geo, frames, k))


def test_a_frame_without_points_inside_the_chain(geo, frames):
    k = 2
    chain = [frames[0], np.zeros((0, 3), np.int32), frames[1], frames[2]]
    blobs = geo.compress(chain, predict="previous")
    assert [b[1] for b in blobs] == [2, 2, 2, 4] and len(blobs[1]) == 24
    got = geo.decompress([_cut(b, k) for b in blobs], lod=k)
    _same(got, chain, k)
    assert got[1].shape == (0, 3)


# ------------------------------------------------------------------ root cubes that differ
def _root_cube_cases():
    rng = np.random.default_rng(12)
    a = np.abs(random_cloud(rng, 700, extent=60, lo=-30)[:, 1:]).astype(np.int32)
    wide, narrow = a * 16 + 64, a[:60] // 8 + 100       # away from the lattice's centre: depths 10 and 2
    return {"a deep frame against a reference of depth < k": (wide, narrow), "a frame of depth < k against a deep reference": (narrow, wide),
            "a reference outside the frame's root cube": (wide, wide + 9000)}


@pytest.mark.parametrize("name", list(_root_cube_cases()))
def test_root_cubes_that_differ(geo, name):
    k = 5
    frame, reference = _root_cube_cases()[name]
    (blob,) = geo.compress([frame], predict="previous", reference=reference)
    d_frame, d_ref = blob[2], ref4.build_tree(reference)[2]
    assert blob[1] == 4
    if "depth < k" in name:
        assert min(d_frame, d_ref) < k < max(d_frame, d_ref)
    (v2,) = _v2_cells(geo, [frame], k)
    for piece in (blob, _cut(blob, k)):
        (cells,) = geo.decompress([piece], lod=k, reference=_cells(reference, k), reference_lod=k)
        assert np.array_equal(cells, _cells(frame, k)) and np.array_equal(cells, v2)
        assert np.array_equal(geo.decompress([piece], lod=k, reference=reference, reference_lod=0)[0], cells)


# ------------------------------------------------------------------ attributes, output forms
@pytest.mark.parametrize("kind", ["scalable", "qstep=16, scalable_to=3"])
def test_attributes_beside_predicted_geometry(geo, frames, kind):
    G, k, chain = pkg().GeometryCodec, 2, frames[:3]
    rng = np.random.default_rng(7)
    attrs = [rng.integers(0, 256, (len(f), 3)).astype(np.uint8) for f in chain]
    kw = dict(scalable=True) if kind == "scalable" else dict(qstep=16, scalable_to=3)
    blobs4, attr4 = geo.compress(chain, attributes=attrs, predict="previous", **kw)
    blobs2, attr2 = geo.compress(chain, attributes=attrs, **kw)
    assert [b[1] for b in blobs4] == [2, 4, 4] and [b[1] for b in blobs2] == [2, 2, 2]

    def cut(blobs, attr_blobs):
        return [_cut(b, k) for b in blobs], [a[:G.attr_lod_info(a, k)[0]] for a in attr_blobs]

    cells4, values4 = geo.decompress(*cut(blobs4, attr4), lod=k)
    cells2, values2 = geo.decompress(*cut(blobs2, attr2), lod=k)
    _same(cells4, chain, k, cells2)
    for f in range(3):
        assert values4[f].shape == (len(cells4[f]), 3) and values4[f].dtype == values2[f].dtype
        assert np.array_equal(values4[f], values2[f]), f


def test_output_forms(geo, frames):
    k, chain = 2, frames[:3]
    cut4 = [_cut(b, k) for b in geo.compress(chain, predict="previous")]
    cut2 = [_cut(b, k) for b in geo.compress(chain)]
    dev = geo.decompress(cut4, lod=k, output="device")
    assert all(d.is_cuda for d in dev)
    _same([d.cpu().numpy() for d in dev], chain, k)
    metric4 = geo.decompress(cut4, lod=k, voxel=0.02)
    metric2 = geo.decompress(cut2, lod=k, voxel=0.02)
    for f in range(3):
        assert metric4[f].dtype == np.float32 and np.array_equal(metric4[f], metric2[f])
        centre = (_cells(chain[f], k).astype(np.float32) * 4 + np.float32(1.5)) * np.float32(0.02)      # exact in float32 up to the product
        assert np.array_equal(metric4[f], centre)


# ------------------------------------------------------------------ what a cut cannot verify
def _either_or(geo, abi, blob, k, m, **kw):
    """the documented contract: PccError, or m rows"""
    try:
        (got,) = geo.decompress([blob], lod=k, **kw)
    except abi.PccError as e:
        return "refused: " + str(e)
    assert got.dtype == np.int32 and got.shape == (m, 3)
    return "%d rows" % m


def test_a_wrong_reference_at_a_cut(geo, frames):
    abi, k, chain = pkg("_abi"), 2, frames[:3]
    blob = _cut(geo.compress(chain, predict="previous")[1], k)
    m = len(_cells(chain[1], k))
    print("another frame's cells:", _either_or(geo, abi, blob, k, m, reference=_cells(chain[2], k), reference_lod=k))
    (got,) = geo.decompress([blob], lod=k, reference=_cells(chain[0], k), reference_lod=k)
    assert np.array_equal(got, _cells(chain[1], k))
    # rows that cannot be cells of the lod (lattice points beyond +-1024 at lod 5) are refused by name
    blob = _cut(geo.compress(chain, predict="previous")[1], 5)
    assert np.abs(chain[0]).max() >= 1024
    err = _refused(geo, abi, [blob], 5, reference=chain[0], reference_lod=5)
    assert err.code == abi.PCC_E_ARG and "cells" in str(err)
    (got,) = geo.decompress([blob], lod=5, reference=_cells(chain[0], 5), reference_lod=5)
    assert np.array_equal(got, _cells(chain[1], 5))


def test_a_damaged_word_above_the_cut(geo, frames):
    abi, k, chain = pkg("_abi"), 2, frames[:3]
    whole = geo.compress(chain, predict="previous")[1]
    blob, h = _cut(whole, k), ref4.header(whole)
    m = len(_cells(chain[1], k))
    bad = bytearray(blob)
    at = h["off_payload"] + 2 * (3 * 64 + 5)             # a word of lane 0's run in chunk 0, which holds the top levels
    assert at + 2 <= len(blob) and struct.unpack_from("<H", blob, h["off_payload"] + 4 * 64)[0] > 5
    bad[at] ^= 0x10
    print("one flipped bit:", _either_or(geo, abi, bytes(bad), k, m, reference=_cells(chain[0], k), reference_lod=k))
    (got,) = geo.decompress([blob], lod=k, reference=_cells(chain[0], k), reference_lod=k)
    assert np.array_equal(got, _cells(chain[1], k))
