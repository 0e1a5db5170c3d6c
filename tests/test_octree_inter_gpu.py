"""Octree blob version 4 on the GPU (csrc/octree4.hip, the <true> forms of csrc/octree2.hip's coder kernels) against
the reference coder of octree_inter_ref.py, byte for byte, and its decoder against np.unique of the frames: the level
boundaries a lane, a chunk and a dword of four nodes can straddle, root cubes that differ, chains of frames, the
combinations with the other keywords of GeometryCodec, damaged blobs, and one full-size sequence.

The decoder reads a format, not this project's encoder (kO4SMax = 256, the smallest S for the chunk count), so one block
of tests decodes blobs of the reference coder under layouts the encoder never writes (octree_inter_ref.encode's smax=
and S=), each test asserting from the blob the property it is there for:
  a word span beyond the LDS window   a half-occupied 64 x 64 x 48 box as one chunk of S = 440: the widest level's lanes
                                      span 12 433 words against kO4Win = 10 240, so k_o4_dec reads the stream in place;
                                      the encoder's own blob of the frame (S = 220, two chunks) spans 7 069
  S at both ends of what o4_parse     23 017 nodes at S = 4 (90 chunks: more than the 64 a wave sums of the chunk table
  accepts                             in one round), S = 8 (45) and S = 512 (1)
  a layout that is not minimal        2 164 nodes at S = 256 and S = 512: one chunk, lanes 9 .. 63 (5 .. 63) without nodes
  a level on a chunk boundary         S = 4: level 11 begins at node 256; a deepest level that begins at node 1 792
  the encoder's second chunk          16 384 nodes (S = 256, one chunk, no slack) and 16 385 (S = 132, two chunks, lanes
                                      61 .. 63 of the second empty), at depth 6 and at depth 16; through the GPU encoder
  damage on these paths               a flipped word, a flipped state and a short chunk on the in-place path, a word in
                                      a lane without nodes, an S rewritten to another the parser accepts: PCC_E_STREAM"""
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


# ------------------------------------------------------------------ layouts and word spans the encoder never emits
K_O4_WIN = 10240      # kO4Win of csrc/octree4.hip: the decoder's window of 16-bit words in LDS


def _decode_only(geo, frame, reference, **layout):
    """a blob of the reference coder under a layout of its own (smax=, S=) through the GPU decoder and the reference
    decoder"""
    blob = ref4.encode(frame, reference, **layout)
    want = _morton_sorted(frame)
    (dec,) = geo.decompress([blob], reference=reference)
    assert dec.dtype == np.int32 and np.array_equal(dec, want), ref4.header(blob)
    assert np.array_equal(ref4.decode(blob, reference), want)
    return blob


def _chunk(blob, c):
    """(byte offset of chunk c, its 64 lane lengths)"""
    h = ref4.header(blob)
    table = struct.unpack_from("<%dI" % h["nc"], blob, h["off_table"])
    at = h["off_payload"] + 2 * sum(table[:c])
    return at, np.array(struct.unpack_from("<64H", blob, at + 2 * 128), np.int64)


def _word_spans(blob):
    """w_hi - w_lo as k_o4_dec forms it, for every launch (level) and every chunk of it: from the first word of the
    first lane that holds a node of the level to the last word of the last such lane"""
    h = ref4.header(blob)
    S = h["S"]
    off = np.cumsum([0] + h["level_n"])
    out = []
    for c in range(h["nc"]):
        _, lens = _chunk(blob, c)
        end = np.cumsum(lens)
        node0 = (64 * c + np.arange(64)) * S
        for L in range(h["depth"]):
            act = np.nonzero(np.maximum(node0, off[L]) < np.minimum(node0 + S, off[L + 1]))[0]
            if len(act):
                out.append(int(end[act[-1]] - (end - lens)[act[0]]))
    return out


_cache = {}


def _half_box():
    """a half-occupied box, the most words a node can cost: 98 051 points, 28 065 nodes, depth 16"""
    if "box" not in _cache:
        g = np.stack(np.meshgrid(np.arange(64), np.arange(64), np.arange(48), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
        rng = np.random.default_rng(7)
        frame = g[rng.random(len(g)) < 0.5] - 32
        reference = g[rng.random(len(g)) < 0.1] - 31
        _cache["box"] = (frame, reference)
    return _cache["box"]


def _scattered():
    """5 999 points, 23 017 nodes, depth 16"""
    if "scattered" not in _cache:
        rng = np.random.default_rng(3)
        frame = np.unique(rng.integers(-150, 150, (6000, 3)), axis=0).astype(np.int32)
        reference = rng.integers(-150, 150, (3000, 3)).astype(np.int32)
        _cache["scattered"] = (frame, reference)
    return _cache["scattered"]


def _checked(geo, key, frame, reference, **layout):
    """_decode_only, once per blob of the module"""
    if key not in _cache:
        _cache[key] = _decode_only(geo, frame, reference, **layout)
    return _cache[key]


def test_word_span_beyond_the_lds_window(geo):
    """one chunk of S = 440 (smax=512): the widest level's lanes span 12 433 words, more than kO4Win = 10 240, so
    k_o4_dec reads the stream in place; the encoder's own layout of the same frame (S = 220, two chunks, 7 069 words)
    stays inside the window"""
    frame, reference = _half_box()
    blob = _checked(geo, "box512", frame, reference, smax=512)
    h = ref4.header(blob)
    assert (h["S"], h["nc"]) == (440, 1), h
    widest = max(_word_spans(blob))
    print("half box, smax=512: S", h["S"], "chunks", h["nc"], "bytes", len(blob), "widest span", widest)
    assert widest > K_O4_WIN, "widest span %d words does not exceed kO4Win = %d: the in-place path is not run" % (widest, K_O4_WIN)
    (own,) = geo.compress([frame], predict="previous", reference=reference)
    assert own == ref4.encode(frame, reference)
    ho = ref4.header(own)
    widest_own = max(_word_spans(own))
    print("half box, the encoder's layout: S", ho["S"], "chunks", ho["nc"], "widest span", widest_own)
    assert ho["nc"] == 2 and 0 < widest_own <= K_O4_WIN, "widest span %d words against kO4Win = %d" % (widest_own, K_O4_WIN)
    assert np.array_equal(geo.decompress([own], reference=reference)[0], _morton_sorted(frame))


@pytest.mark.parametrize("S", [4, 8, 512])
def test_s_at_the_ends_and_more_than_64_chunks(geo, S):
    """S = 4: 90 chunks, so the sum of the chunk table in front of a chunk takes a second round of the wave"""
    frame, reference = _scattered()
    h = ref4.header(_checked(geo, "scattered%d" % S, frame, reference, S=S))
    n_nodes = sum(h["level_n"])
    print("scattered: nodes", n_nodes, "S", S, "chunks", h["nc"])
    assert h["S"] == S and h["nc"] == -(-n_nodes // (64 * S))
    if S == 4:
        assert h["nc"] > 64
    if S == 512:
        assert h["nc"] == 1


@pytest.mark.parametrize("S", [256, 512])
def test_a_layout_that_is_not_minimal(geo, S):
    """about 2k nodes dealt 256 or 512 to a lane: one chunk whose lanes from 9 (5) on hold no node"""
    frame, reference = _boundary_cloud(0), _boundary_cloud(100)
    blob = _checked(geo, "sparse%d" % S, frame, reference, S=S)
    h = ref4.header(blob)
    n_nodes = sum(h["level_n"])
    assert h["nc"] == 1 and 8 * 256 < n_nodes <= 9 * 256      # lanes 9 .. 63 of S = 256 begin behind the last node
    _, lens = _chunk(blob, 0)
    assert np.all(lens[-(-n_nodes // S):] == 0) and np.all(lens[:-(-n_nodes // S)] > 0)


# as BOUNDARY_SEEDS, the same search: the first cloud with a level (beyond the first two) that begins at node 256, the
# first node of chunk 1 under S = 4, and the first cloud whose DEEPEST level begins at a chunk's first node under S = 4 or 8
CHUNK_BOUNDARY_SEEDS = {"level 11 begins at node 256 = 64 * 4": (18, 4), "the deepest level begins at node 1792 = 7 * 64 * 4": (40, 4)}


@pytest.mark.parametrize("name", list(CHUNK_BOUNDARY_SEEDS))
def test_a_level_on_a_chunk_boundary(geo, name):
    """the lane in front of the boundary ends its run and leaves nothing behind, the launch of the level begins at a
    chunk's own states"""
    seed, S = CHUNK_BOUNDARY_SEEDS[name]
    frame = _boundary_cloud(seed)
    levels, _, depth, _, _ = ref4.build_tree(frame)
    off = np.cumsum([0] + [len(lv) for lv in levels])
    if "deepest" in name:
        assert off[depth - 1] % (64 * S) == 0 and off[depth - 1] == 1792
    else:
        assert any(off[L] % (64 * S) == 0 for L in range(2, depth)) and off[11] == 256
    _decode_only(geo, frame, _boundary_cloud(seed + 100), S=S)


# prefixes of one shuffled cloud, found by bisection on the CPU with octree_inter_ref.build_tree: the longest with
# 16 384 nodes (one chunk of S = 256, every lane full) and the next (two chunks of S = 132, the last lanes empty); under
# the shift the cube straddles the origin (depth 16) and ten levels of one node move the prefixes
CHUNK_SWITCH = {"depth 6": (0, 14260, 14261), "depth 16": (-32, 14153, 14154)}


@pytest.mark.parametrize("delta", [0, 1])
@pytest.mark.parametrize("name", list(CHUNK_SWITCH))
def test_either_side_of_the_encoders_second_chunk(geo, name, delta):
    shift, full, _ = CHUNK_SWITCH[name]
    assert CHUNK_SWITCH[name][2] == full + 1
    rng = np.random.default_rng(1)
    pts = np.unique(rng.integers(0, 64, (26000, 3)), axis=0).astype(np.int32)
    pts = pts[rng.permutation(len(pts))]
    frame, reference = pts[:full + delta] + shift, pts[20000:] + 1
    levels, _, depth, _, _ = ref4.build_tree(frame)
    n_nodes = sum(len(lv) for lv in levels)
    assert depth == int(name.split()[1]) and n_nodes == 16384 + delta
    blob = _pair(geo, frame, reference)
    h = ref4.header(blob)
    assert (h["S"], h["nc"]) == ((256, 1), (132, 2))[delta]
    _, lens = _chunk(blob, h["nc"] - 1)
    if delta:      # chunk 1: 7 937 nodes, 60 lanes of 132 and one of 17; lanes 61 .. 63 hold none
        assert np.all(lens[61:] == 0) and np.all(lens[:61] > 0)
    else:
        assert np.all(lens > 0)


def test_damaged_blobs_on_the_new_paths(geo):
    """as test_damaged_blobs_are_errors, on blobs that run the in-place word path, a lane without nodes and a layout
    of another S: PCC_E_STREAM, and the call after it decodes"""
    abi = pkg("_abi")
    G = type(geo)

    def flip(blob, at, bit=0x10):
        b = bytearray(blob)
        b[at] ^= bit
        return bytes(b)

    def refused(name, bad, blob, frame, reference):
        with pytest.raises(abi.PccError) as e:
            geo.decompress([bad], reference=reference)
            pytest.fail(name + " decoded")
        assert e.value.code == abi.PCC_E_STREAM, (name, str(e.value))
        assert np.array_equal(geo.decompress([blob], reference=reference)[0], _morton_sorted(frame)), name

    # the blob whose widest span is read in place
    frame, reference = _half_box()
    blob = _checked(geo, "box512", frame, reference, smax=512)
    assert max(_word_spans(blob)) > K_O4_WIN
    h = ref4.header(blob)
    at, lens = _chunk(blob, 0)
    assert lens[30] > 100
    shortened = bytearray(blob)      # the chunk one word shorter, the tables left as they are
    del shortened[at + 2 * 192:at + 2 * 192 + 2]
    struct.pack_into("<I", shortened, 20, len(shortened) - 24)
    cases = {"a flipped payload word in lane 30's run": flip(blob, at + 2 * (192 + int(lens[:30].sum()) + 40)),
             "a flipped state": flip(blob, at + 1), "a shortened chunk": bytes(shortened)}
    for name, bad in cases.items():
        refused(name, bad, blob, frame, reference)

    # a lane without nodes that announces a word: the parser has nothing against it
    frame, reference = _boundary_cloud(0), _boundary_cloud(100)
    blob = _checked(geo, "sparse256", frame, reference, S=256)
    h = ref4.header(blob)
    at, lens = _chunk(blob, 0)
    assert h["nc"] == 1 and 63 * 256 >= sum(h["level_n"]) and lens[62] == 0 and lens[63] == 0
    bad = bytearray(blob) + struct.pack("<H", 0x1234)
    struct.pack_into("<H", bad, at + 2 * (128 + 63), 1)
    struct.pack_into("<I", bad, h["off_table"], struct.unpack_from("<I", blob, h["off_table"])[0] + 1)
    struct.pack_into("<I", bad, 20, len(bad) - 24)
    assert G.geometry_info(bytes(bad)) == G.geometry_info(blob)
    refused("a word in a lane without nodes", bytes(bad), blob, frame, reference)

    # another S in the header that the parser accepts: every node is dealt to another lane
    def another_s(blob, S):
        h = ref4.header(blob)
        n_nodes = sum(h["level_n"])
        assert S != h["S"] and S % 4 == 0 and 64 * S * (h["nc"] - 1) < n_nodes <= 64 * S * h["nc"]
        b = bytearray(blob)
        struct.pack_into("<I", b, 24 + 4 * h["depth"], S)
        assert G.geometry_info(bytes(b)) == G.geometry_info(blob)
        return bytes(b)

    # (the 45 chunks of S = 8 and the 90 of S = 4 of the scattered frame admit no other S; its one chunk of S = 512
    # admits 360 .. 508)
    frame, reference = _scattered()
    blob = _checked(geo, "scattered512", frame, reference, S=512)
    for S in (360, 508):
        refused("S = 512 rewritten to %d" % S, another_s(blob, S), blob, frame, reference)
    frame, reference = _boundary_cloud(0)[:160], _boundary_cloud(100)      # 881 nodes: two chunks under S = 8 and under S = 12
    blob = _checked(geo, "small8", frame, reference, S=8)
    assert ref4.header(blob)["nc"] == 2
    refused("S = 8 rewritten to 12", another_s(blob, 12), blob, frame, reference)


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
