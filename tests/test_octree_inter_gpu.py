"""Octree blob version 4 on the GPU (csrc/octree4.hip, the <true> forms of csrc/octree2.hip's coder kernels) against
the reference coder of octree_inter_ref.py, byte for byte, and its decoder against np.unique of the frames: the level
boundaries a lane, a chunk and a dword of four nodes can straddle, root cubes that differ, chains of frames, the
combinations with the other keywords of GeometryCodec, damaged blobs, and one full-size sequence."""
import struct

import numpy as np
import pytest

import octree_inter_ref as ref4
from conftest import pkg, random_cloud
from test_geometry_calls import EXPECTED, inputs, recorded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo(rt):
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _unique(p):
    return np.unique(np.asarray(p, np.int32), axis=0)


def _morton_sorted(p):
    p = _unique(p)
    return p[np.argsort(ref4.morton(p.astype(np.int64) + 32768), kind="stable")]


def _pair(geo, frame, reference):
    """the blob of `frame` coded against `reference`, checked against the reference coder and decoded again"""
    (blob,) = geo.compress([frame], predict="previous", reference=reference)
    assert blob == ref4.encode(frame, reference), (len(blob), blob[:4])
    (dec,) = geo.decompress([blob], reference=reference)
    assert dec.dtype == np.int32 and np.array_equal(dec, _morton_sorted(frame))
    return blob


@pytest.fixture(scope="module")
def sweeps(wl):
    return [f["points"].astype(np.int32) for f in wl.lidar_sequence(2, 16, 600)]


def test_the_sweep_pair(geo, sweeps):
    """two chunks (S = 232 at 29.7k nodes): level boundaries inside lanes and inside a chunk"""
    import torch
    f0, f1 = sweeps
    blob = _pair(geo, f1, f0)
    h = ref4.header(blob)
    assert h["nc"] == 2 and h["S"] <= 256 and h["ref_n"] == len(_unique(f0))
    (dev,) = geo.decompress([blob], output="device", reference=torch.from_numpy(f0).to(geo.rt.device))
    assert np.array_equal(dev.cpu().numpy(), _morton_sorted(f1))
    # a reference in another row order and with repeated rows is the same reference
    rng = np.random.default_rng(0)
    shuffled = np.concatenate([f0, f0[:50]])[rng.permutation(len(f0) + 50)]
    assert np.array_equal(geo.decompress([blob], reference=shuffled)[0], _morton_sorted(f1))


def _root_cube_cases():
    rng = np.random.default_rng(12)
    a = random_cloud(rng, 700, extent=60, lo=-30)[:, 1:]
    return {
        "small frame inside a large reference": (a[:60] // 4, a * 20),
        "large frame around a small reference": (a * 20, a[:60] // 4),
        "reference outside the root cube": (a, a + 5000),
        "depth 16": (np.concatenate([a, [[-32767] * 3, [32767] * 3]]), np.concatenate([a + 1, [[32767] * 3, [-32767, 0, 0]]])),
    }


@pytest.mark.parametrize("name", list(_root_cube_cases()))
def test_root_cubes_that_differ(geo, name):
    frame, reference = _root_cube_cases()[name]
    blob = _pair(geo, frame.astype(np.int32), reference.astype(np.int32))
    if name == "depth 16":
        assert blob[2] == 16


@pytest.mark.parametrize("n", [1, 2, 9])
def test_frames_of_a_few_points(geo, n):
    rng = np.random.default_rng(n)
    a = random_cloud(rng, 40, extent=30, lo=-15)[:, 1:].astype(np.int32)
    _pair(geo, a[:n], a[n - 1:])


@pytest.mark.parametrize("delta", [0, 1])
def test_either_side_of_the_single_workgroup_level_builder(geo, delta):
    """65536 leaves (pcc_octree_small_max(), csrc/octree.hip) and one more: both forms of the levels; a dense block keeps
    the Python coder quick"""
    n = 65536 + delta
    g = np.stack(np.meshgrid(*[np.arange(41)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    assert len(g) >= n
    rng = np.random.default_rng(5)
    frame = g[rng.permutation(len(g))[:n]] - 20
    reference = g[rng.permutation(len(g))[:30000]] - 19
    _pair(geo, frame, reference)


# found by a seeded search on the CPU with octree_inter_ref.build_tree over _boundary_cloud(seed), seeds 0, 1, 2, ..:
# the first cloud with a level (beyond the first two) that begins at a lane's first node, and the first clouds whose
# deepest level begins at a node = 1, 2, 3 mod 4 (a dword of four occupancy bytes then belongs to two levels)
BOUNDARY_SEEDS = {"a level begins at a lane's first node": 0, "deepest level at 1 mod 4": 2, "deepest level at 2 mod 4": 3,
                  "deepest level at 3 mod 4": 1}


def _boundary_cloud(seed):
    rng = np.random.default_rng(seed)
    return np.unique(rng.integers(-150, 150, (400, 3)), axis=0).astype(np.int32)


@pytest.mark.parametrize("name", list(BOUNDARY_SEEDS))
def test_level_boundaries(geo, name):
    frame = _boundary_cloud(BOUNDARY_SEEDS[name])
    levels, _, depth, _, _ = ref4.build_tree(frame)
    off = np.cumsum([0] + [len(lv) for lv in levels])
    S, _ = ref4._layout(int(off[-1]), 256)
    if "lane" in name:      # the property the seed was found for
        assert any(off[L] % S == 0 for L in range(2, depth))
    else:
        assert off[depth - 1] % 4 == int(name.split()[3])
    _pair(geo, frame, _boundary_cloud(BOUNDARY_SEEDS[name] + 100))


# ------------------------------------------------------------------ chains
@pytest.fixture(scope="module")
def chain():
    rng = np.random.default_rng(21)
    base = random_cloud(rng, 1500, extent=90, lo=-45)[:, 1:].astype(np.int32)
    return [np.concatenate([base[40 * f:1200 + 40 * f], base[:30]]) + np.array([f, 0, 0], np.int32) for f in range(6)]


@pytest.mark.parametrize("period", [3, None])
def test_chain_of_six_frames(geo, chain, period):
    PccError = pkg("_abi").PccError
    G = type(geo)
    blobs = geo.compress(chain, predict="previous", intra_period=period)
    intra = [f % period == 0 if period else f == 0 for f in range(6)]
    assert [G.geometry_info(b)["version"] for b in blobs] == [2 if i else 4 for i in intra]
    assert [G.geometry_info(b)["predicted"] for b in blobs] == [not i for i in intra]
    plain = geo.compress(chain)
    for f in range(6):
        want = plain[f] if intra[f] else ref4.encode(chain[f], chain[f - 1])
        assert blobs[f] == want, f
        if not intra[f]:
            assert G.geometry_info(blobs[f])["reference_points"] == len(_unique(chain[f - 1]))
    want = [_morton_sorted(f) for f in chain]
    got = geo.decompress(blobs)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    if period == 3:      # blob 3 is a random-access point
        assert all(np.array_equal(a, b) for a, b in zip(geo.decompress(blobs[3:]), want[3:]))
    else:
        with pytest.raises(PccError, match="frame 0"):
            geo.decompress(blobs[3:])
    got = geo.decompress(blobs[1:], reference=chain[0])
    assert all(np.array_equal(a, b) for a, b in zip(got, want[1:]))
    with pytest.raises(PccError, match="frame 0") as e:
        geo.decompress(blobs[1:])
    assert e.value.code == pkg("_abi").PCC_E_ARG
    with pytest.raises(PccError, match="frame 0") as e:      # another point count
        geo.decompress(blobs[1:], reference=chain[0][100:])
    assert e.value.code == pkg("_abi").PCC_E_ARG
    moved = chain[0].copy()
    moved[500, 2] += 1      # the same count, another set
    if len(_unique(moved)) == len(_unique(chain[0])):
        with pytest.raises(PccError, match="frame 0") as e:
            geo.decompress(blobs[1:], reference=moved)
        assert e.value.code == pkg("_abi").PCC_E_ARG
    # one frame per call against the last, as a streaming sender codes
    (one,) = geo.compress([chain[1]], predict="previous", reference=chain[0])
    assert one == blobs[1]
    assert all(np.array_equal(a, b) for a, b in zip(geo.decompress(blobs), want))      # the codec stays usable


def test_an_empty_frame_in_the_middle(geo, chain):
    G = type(geo)
    frames = [chain[0], chain[1], np.zeros((0, 3), np.int32), chain[3], chain[4]]
    blobs = geo.compress(frames, predict="previous")
    assert [G.geometry_info(b)["version"] for b in blobs] == [2, 4, 2, 2, 4] and len(blobs[2]) == 24
    assert blobs[3] == geo.compress([chain[3]])[0]
    got = geo.decompress(blobs)
    assert all(np.array_equal(a, _morton_sorted(f).reshape(-1, 3)) for a, f in zip(got, frames))


# ------------------------------------------------------------------ combinations
def test_lod_on_the_senders_side(geo, chain):
    f0, f1 = chain[0] * 5, chain[1] * 5
    blobs = geo.compress([f0, f1], lod=2, predict="previous")
    assert blobs[1] == ref4.encode(f1 >> 2, f0 >> 2, bias=32768 >> 2)
    got = geo.decompress(blobs)
    assert np.array_equal(got[1], geo.decompress(geo.compress([f1], lod=2))[0])


def test_float32_frames_with_voxel_and_drop(geo, chain):
    voxel = 0.5
    fl = [(f.astype(np.float32) * np.float32(voxel)) for f in chain[:3]]
    fl[1] = np.concatenate([fl[1][:10], np.full((4, 3), np.nan, np.float32), fl[1][10:]])
    blobs = geo.compress(fl, voxel=voxel, invalid="drop", predict="previous")
    assert blobs == geo.compress(chain[:3], predict="previous")
    got = geo.decompress(blobs, voxel=voxel)
    assert got[2].dtype == np.float32 and np.array_equal(got[2], _morton_sorted(chain[2]).astype(np.float32) * np.float32(voxel))


def test_return_index(geo, chain):
    frames = chain[:3]
    blobs, index = geo.compress(frames, predict="previous", return_index=True)
    plain, plain_index = geo.compress(frames, return_index=True)
    dec = geo.decompress(blobs)
    for f in range(3):
        assert np.array_equal(index[f], plain_index[f]) and np.array_equal(dec[f][index[f]], frames[f])


@pytest.mark.parametrize("kw", [{}, {"qstep": 16}])
def test_attributes_beside_predicted_geometry(geo, chain, kw):
    rng = np.random.default_rng(4)
    frames = chain[:3]
    attrs = [rng.integers(0, 256, (f.shape[0], 3)).astype(np.uint8) for f in frames]
    blobs, ab = geo.compress(frames, attributes=attrs, predict="previous", **kw)
    plain, plain_ab = geo.compress(frames, attributes=attrs, **kw)
    assert ab == plain_ab and blobs[0] == plain[0] and blobs[1] != plain[1]
    pts, vals = geo.decompress(blobs, ab)
    ppts, pvals = geo.decompress(plain, plain_ab)
    assert all(np.array_equal(a, b) for a, b in zip(pts, ppts)) and all(np.array_equal(a, b) for a, b in zip(vals, pvals))


# ------------------------------------------------------------------ damaged blobs
def test_damaged_blobs_are_errors(geo, chain):
    """as test_hip_v2_corrupt_blobs_are_errors for version 2: an error, and the call after it decodes"""
    PccError = pkg("_abi").PccError
    ref, frame = chain[0], chain[1]
    (blob,) = geo.compress([frame], predict="previous", reference=ref)
    h = ref4.header(blob)
    want = _morton_sorted(frame)

    def flip(at, bit=0x10):
        b = bytearray(blob)
        b[at] ^= bit
        return bytes(b)

    def shortened():      # the first chunk one word shorter, the tables left as they are
        b = bytearray(blob)
        del b[h["off_payload"] + 2 * 192:h["off_payload"] + 2 * 192 + 2]
        struct.pack_into("<I", b, 20, len(b) - 24)
        return bytes(b)
    level_off = bytearray(blob)
    struct.pack_into("<I", level_off, 24 + 4 * (h["depth"] - 2), h["level_n"][-2] + 1)
    ref_off = bytearray(blob)
    struct.pack_into("<I", ref_off, 24 + 4 * h["depth"] + 8, h["ref_n"] + 1)
    sum_off = bytearray(blob)
    sum_off[24 + 4 * h["depth"] + 12] ^= 1
    cases = {"a flipped payload word": flip(h["off_payload"] + 2 * 192 + 40), "a flipped state": flip(h["off_payload"] + 1),
             "a shortened chunk": shortened(), "a level size off by one": bytes(level_off), "ref_n off by one": bytes(ref_off),
             "ref_sum off by one": bytes(sum_off), "a truncated blob": blob[:-2]}
    for name, bad in cases.items():
        with pytest.raises(PccError):
            geo.decompress([bad], reference=ref)
            pytest.fail(name + " decoded")
        assert np.array_equal(geo.decompress([blob], reference=ref)[0], want), name


# ------------------------------------------------------------------ full size, and the defaults
def test_full_size_sequence(geo, wl):
    frames = [f["points"] for f in wl.lidar_sequence(3, 64, 1800, velocity=(10, 0, 0))]
    blobs = geo.compress(frames, predict="previous")
    assert blobs == geo.compress(frames, predict="previous")
    plain = geo.compress(frames)
    assert blobs[0] == plain[0] and all(len(b) < len(p) for b, p in zip(blobs[1:], plain[1:]))
    print("full-size sweeps, bytes of version 2 / 4:", [(len(p), len(b)) for b, p in zip(blobs, plain)])
    got = geo.decompress(blobs)
    assert all(np.array_equal(a, _morton_sorted(f)) for a, f in zip(got, frames))


def test_the_defaults_make_the_calls_of_before(geo):
    x = inputs()
    blobs, calls = recorded(geo, lambda: geo.compress(x["ints"]))
    assert calls == EXPECTED["integer host"]
    _, calls = recorded(geo, lambda: geo.decompress(blobs))
    assert [c[0] for c in calls] == ["pcc_octree_decode_frames"] * 2      # the sizes, then the points
