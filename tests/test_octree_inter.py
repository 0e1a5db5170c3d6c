"""Octree blob version 4, a predicted frame (include/pcc.h has the rule; csrc/octree4.hip, csrc/octree4_blob.h).  CPU
part: the reference coder of octree_inter_ref.py against itself (its decoder inverts its encoder; with the context
split taken out its payload is the version-2 coder's of test_octree2.py), against streams worked by hand, and the two
properties of the rule that make it worth having: a frame equal to its reference costs almost nothing, and a LiDAR
sweep coded against the sweep before it is well below its version-2 blob.  Then the host-only interfaces: the argument
checks of GeometryCodec's new keywords and geometry_info."""
import struct

import numpy as np
import pytest

import octree_inter_ref as ref4
from conftest import pkg, random_cloud
from test_octree2 import py_octree2_encode

CTX4 = 324


def _cases():
    rng = np.random.default_rng(11)
    a = random_cloud(rng, 900, extent=60, lo=-30)[:, 1:]
    yield "same set", a, a
    yield "shifted by one", a, a + np.array([1, 0, 0])
    yield "small frame inside a large reference", a[:40] // 4, a * 20
    yield "large frame around a small reference", a * 20, a[:40] // 4
    yield "reference outside the root cube", a, a + 5000
    yield "one point", np.array([[3, -4, 5]]), np.array([[3, -4, 5], [9, 9, 9]])
    yield "two points", np.array([[3, -4, 5], [3, -4, 6]]), np.array([[3, -4, 6]])
    yield "nine points", a[:9], a[4:30]
    yield "depth 16", np.array([[-32767, -32767, -32767], [32767, 32767, 32767], [0, 0, 0], [5, 5, 5]]), \
        np.array([[32767, 32767, 32767], [0, 0, 1], [-32768, 0, 0]])
    yield "more than one chunk", random_cloud(rng, 7000, extent=4000, lo=-2000)[:, 1:], random_cloud(rng, 3000, extent=4000, lo=-2000)[:, 1:]


@pytest.mark.parametrize("name", [c[0] for c in _cases()])
def test_reference_decoder_inverts_its_encoder(name):
    _, pts, ref = next(c for c in _cases() if c[0] == name)
    blob = ref4.encode(pts, ref)
    dec = ref4.decode(blob, ref)
    want = np.unique(pts, axis=0)
    assert dec.shape == want.shape and np.array_equal(np.unique(dec, axis=0), want)
    # Morton order, as every decoder of this project returns points
    assert np.all(np.diff(ref4.morton(dec + 32768)) > 0)
    with pytest.raises(ValueError):
        ref4.decode(blob, np.concatenate([ref, [[77, 77, 77]]]))


@pytest.mark.parametrize("name", [c[0] for c in _cases()])
def test_without_the_context_split_the_payload_is_version_2s(name):
    _, pts, ref = next(c for c in _cases() if c[0] == name)
    v2 = py_octree2_encode(pts, 32768)
    mine = ref4.encode(pts, ref, split=False, smax=512)
    depth = v2[2]
    at = 24 + 4 * depth + 8                                    # behind S and the chunk count
    assert mine[2:20] == v2[2:20] and mine[24:at] == v2[24:at]   # depth, n, origin; level sizes, S, chunks
    assert mine[at + 12:] == v2[at:]                           # p0[108], chunk table, chunks: only ref_n and ref_sum lie between


def _kat(p0_ctx_zero, p0_ctx_one, ref_n, ref_sum):
    """the blob of the one point (3, -4, 5) of test_octree2's known answer: one node of byte 0x20, whose eight decisions
    see the same probabilities whatever contexts they fall into — seven contexts that saw one zero (p0 = 1024), one
    that saw one one (3072), the others 2048 — so lane 0's state is version 2's 649216 = 0x0009E800 and no word is
    emitted"""
    p0 = [2048] * CTX4
    for k in p0_ctx_zero:
        p0[k] = 1024
    p0[p0_ctx_one] = 3072
    states = [0xE800, 0x0009] + [0x0000, 0x0001] * 63
    body = struct.pack("<I", 1) + struct.pack("<II", 4, 1) + struct.pack("<IQ", ref_n, ref_sum)
    body += struct.pack("<324H", *p0) + struct.pack("<I", 192) + struct.pack("<128H", *states) + struct.pack("<64H", *([0] * 64))
    return bytes([ord("O"), 4, 1, 0]) + struct.pack("<I", 1) + struct.pack("<3i", 2, -4, 4) + struct.pack("<I", len(body)) + body


def test_known_answer_one_point_against_one_point():
    """Worked by hand.  The frame is test_octree2's one point (3, -4, 5): root cube of depth 1 at (2, -4, 4), octant 5,
    one node of byte 0x20 in level class 0; version 2 codes zeros at contexts 0, 1, 3, 6, 10 (j = 0 .. 4, no one yet), the
    one at 15 (j = 5), zeros at 22 and 29 (j = 6, 7, one one so far).
    Reference (3, -4, 5), the same cell: the reference byte is 0x20 as well, so r = 2 at j = 5 and r = 1 elsewhere:
    the zeros at 108 + {0, 1, 3, 6, 10, 22, 29}, the one at 216 + 15.  ref_sum = 3 << 32 | 0xFFFC << 16 | 5.
    Reference (2, -4, 4), the cube's corner cell, octant 0: reference byte 0x01, r = 2 at j = 0 and 1 elsewhere: the
    zeros at 216 + 0 and 108 + {1, 3, 6, 10, 22, 29}, the one at 108 + 15.  ref_sum = 2 << 32 | 0xFFFC << 16 | 4.
    Reference (100, 100, 100), outside the root cube: reference byte 0, version 2's contexts."""
    pt = np.array([[3, -4, 5]])
    same = _kat([108 + k for k in (0, 1, 3, 6, 10, 22, 29)], 216 + 15, 1, (3 << 32) | (0xFFFC << 16) | 5)
    assert ref4.encode(pt, np.array([[3, -4, 5]])) == same
    other = _kat([216] + [108 + k for k in (1, 3, 6, 10, 22, 29)], 108 + 15, 1, (2 << 32) | (0xFFFC << 16) | 4)
    assert ref4.encode(pt, np.array([[2, -4, 4]])) == other
    outside = _kat([0, 1, 3, 6, 10, 22, 29], 15, 1, (100 << 32) | (100 << 16) | 100)
    assert ref4.encode(pt, np.array([[100, 100, 100]])) == outside
    for blob, r in ((same, [[3, -4, 5]]), (other, [[2, -4, 4]]), (outside, [[100, 100, 100]])):
        assert np.array_equal(ref4.decode(blob, np.array(r)), pt)


def test_header_fields():
    rng = np.random.default_rng(2)
    pts = random_cloud(rng, 500, extent=100, lo=-50)[:, 1:]
    ref = pts[:123] + 1
    blob = ref4.encode(pts, ref)
    h = ref4.header(blob)
    levels, _, depth, org, n = ref4.build_tree(pts)
    assert blob[:4] == bytes([ord("O"), 4, depth, 0]) and h["n"] == n == 500 and h["origin"] == tuple(int(v) - 32768 for v in org)
    assert h["payload"] == len(blob) - 24 and h["level_n"] == [len(lv) for lv in levels]
    n_nodes = sum(h["level_n"])
    assert h["nc"] == 1 and h["S"] == -(-(-(-n_nodes // 64)) // 4) * 4 and h["S"] <= 256
    assert h["ref_n"] == 123 and h["ref_sum"] == ref4.Reference(ref).sum
    p0 = struct.unpack_from("<324H", blob, h["off_p0"])
    assert all(16 <= p <= 4080 for p in p0)
    assert struct.unpack_from("<I", blob, h["off_table"])[0] * 2 == len(blob) - h["off_payload"]
    # the layout bound of its own: 256 nodes per lane where version 2 deals 512
    big = ref4.encode(random_cloud(rng, 6000, extent=4000, lo=-2000)[:, 1:], ref)
    hb = ref4.header(big)
    assert hb["nc"] == -(-sum(hb["level_n"]) // (64 * 256)) >= 2 and hb["S"] <= 256 and hb["S"] % 4 == 0


# ------------------------------------------------------------------ layouts the format allows and the encoder never chooses
def _small_frame():
    """about 1.5k nodes at depth 16"""
    rng = np.random.default_rng(14)
    a = np.unique(rng.integers(-150, 150, (420, 3)), axis=0)
    return a[:270], a[200:]


@pytest.mark.parametrize("S", [4, 8, 64, 132, 512])
def test_forced_layout_round_trip(S):
    """S = 64 is not minimal for this frame (24 lanes of one chunk would do with S = 24): lanes 24 .. 63 hold no node"""
    pts, ref = _small_frame()
    blob = ref4.encode(pts, ref, S=S)
    h = ref4.header(blob)
    n_nodes = sum(h["level_n"])
    assert 1400 <= n_nodes <= 1600
    assert h["S"] == S and h["nc"] == max(1, -(-n_nodes // (64 * S)))
    assert {4: h["nc"] > 1, 8: h["nc"] > 1, 64: h["nc"] == 1 and -(-n_nodes // 64) < 64, 132: h["nc"] == 1, 512: h["nc"] == 1}[S]
    dec = ref4.decode(blob, ref)
    assert np.array_equal(np.unique(dec, axis=0), pts) and np.all(np.diff(ref4.morton(dec + 32768)) > 0)
    # a lane whose first node lies behind the last: the initial state and no words
    words = struct.unpack_from("<192H", blob, h["off_payload"] + 2 * sum(struct.unpack_from("<%dI" % (h["nc"] - 1), blob, h["off_table"])))
    for lane in range(64):
        if (64 * (h["nc"] - 1) + lane) * S >= n_nodes:
            assert words[2 * lane:2 * lane + 2] == (0, 1) and words[128 + lane] == 0


def test_forced_layout_of_the_encoders_own_choice_is_the_same_blob():
    pts, ref = _small_frame()
    for frame in (pts, pts[:9], random_cloud(np.random.default_rng(6), 7000, extent=4000, lo=-2000)[:, 1:]):
        n_nodes = sum(len(lv) for lv in ref4.build_tree(frame)[0])
        S0, nc0 = ref4._layout(n_nodes, 256)
        blob = ref4.encode(frame, ref)
        assert ref4.encode(frame, ref, S=S0) == blob and (ref4.header(blob)["S"], ref4.header(blob)["nc"]) == (S0, nc0)
    assert ref4.encode(pts, ref, smax=512, S=None) == ref4.encode(pts, ref, smax=512)


@pytest.mark.parametrize("S", [0, 2, 6, 516, -4, 4.5])
def test_forced_layout_outside_the_format_is_refused(S):
    pts, ref = _small_frame()
    with pytest.raises(ValueError, match="multiple of 4"):
        ref4.encode(pts, ref, S=S)


def test_the_parsers_boundary_of_S_and_the_chunk_count():
    """o4_parse through geometry_info: S any multiple of 4 in 4 .. 512 with 64 S (nc - 1) < nodes <= 64 S nc"""
    G = _geo_class()
    PccError = pkg("_abi").PccError
    pts, ref = _small_frame()
    n_nodes = sum(len(lv) for lv in ref4.build_tree(pts)[0])
    want = {"version": 4, "points": len(pts), "predicted": True, "reference_points": len(ref)}
    for S in (4, 512):
        assert G.geometry_info(ref4.encode(pts, ref, S=S)) == want

    def rewritten(blob, S=None, nc=None):
        b, h = bytearray(blob), ref4.header(blob)
        struct.pack_into("<II", b, 24 + 4 * h["depth"], h["S"] if S is None else S, h["nc"] if nc is None else nc)
        return bytes(b)

    def refused(bad):
        with pytest.raises(PccError) as e:
            G.geometry_info(bad)
        assert e.value.code == pkg("_abi").PCC_E_STREAM

    one = ref4.encode(pts, ref, S=512)                    # one chunk
    assert ref4.header(one)["nc"] == 1 and n_nodes <= 64 * 24
    for S in (0, 2, 6, 516, 1 << 31, (1 << 32) - 4):
        refused(rewritten(one, S=S))
    for S in (24, 28, 256, 508):                          # one chunk of any S that holds the nodes: the table is still one entry
        assert G.geometry_info(rewritten(one, S=S)) == want
    refused(rewritten(one, S=20))                         # 64 * 20 < nodes: one chunk does not hold them
    refused(rewritten(one, nc=0))
    refused(rewritten(one, nc=2))
    many = ref4.encode(pts, ref, S=4)
    nc = ref4.header(many)["nc"]
    assert nc == -(-n_nodes // 256) >= 5
    refused(rewritten(many, nc=nc - 1))
    refused(rewritten(many, nc=nc + 1))
    refused(rewritten(many, S=8))                         # 64 * 8 * (nc - 1) >= nodes: the last chunk would hold none
    assert 64 * 8 * (nc - 1) >= n_nodes


def test_ref_sum_of_three_points_by_hand():
    """(1, 2, 3) -> 0x0001_0002_0003; (-1, 0, 32767) -> 0xFFFF_0000_7FFF; (-32768, 5, -2) -> 0x8000_0005_FFFE;
    the first two add to 0x1_0000_0002_8002, the third makes 0x1_8000_0008_8000"""
    r = ref4.Reference(np.array([[1, 2, 3], [-1, 0, 32767], [-32768, 5, -2], [1, 2, 3]]))
    assert r.n == 3 and r.sum == (0x18000 << 32) | 0x00088000


def test_a_frame_equal_to_its_reference_costs_almost_nothing(oracle, wl):
    """every decision falls into a context that always sees the same bit, so only the probability floor (0.0056 bit
    per decision) and the fixed tables remain"""
    pts = wl.lidar_sequence(1, 16, 600)[0]["points"].astype(np.int32)
    assert len(np.unique(pts, axis=0)) >= 8000
    v2 = oracle.octree_encode(pts, 32768, version=2)
    v4 = ref4.encode(pts, pts)
    print("identical frame: version 2", len(v2), "bytes, version 4", len(v4))
    assert len(v4) < len(v2) / 4
    assert np.array_equal(ref4.decode(v4, pts), oracle.octree_decode(v2))


def test_a_sweep_against_the_sweep_before_it(oracle, wl):
    f0, f1 = [f["points"].astype(np.int32) for f in wl.lidar_sequence(2, 16, 600)]
    v2 = oracle.octree_encode(f1, 32768, version=2)
    v4 = ref4.encode(f1, f0)
    print("sweep 1 against sweep 0: version 2", len(v2), "bytes, version 4", len(v4), "ratio %.3f" % (len(v4) / len(v2)))
    assert len(v4) < 0.8 * len(v2)
    assert np.array_equal(ref4.decode(v4, f0), oracle.octree_decode(v2))


def test_lidar_sequence_workload(wl):
    a = wl.lidar_sequence(3, 8, 200, seed=4, velocity=(10, 0, 0))
    b = wl.lidar_sequence(3, 8, 200, seed=4, velocity=(10, 0, 0))
    assert len(a) == 3 and all(np.array_equal(x["points"], y["points"]) for x, y in zip(a, b))
    assert all(f["points"].dtype == np.int16 and f["points"].shape[1] == 3 for f in a)
    still = wl.lidar_sequence(2, 8, 200, seed=4)
    assert not np.array_equal(still[0]["points"], still[1]["points"])      # each frame its own noise
    assert not np.array_equal(a[1]["points"], still[1]["points"])          # the sensor moved


# ------------------------------------------------------------------ host-only interfaces
def _geo_class():
    return pkg("geometry").GeometryCodec


def test_geometry_info_on_v2_v4_empty_and_truncated_blobs(oracle):
    G = _geo_class()
    PccError = pkg("_abi").PccError
    rng = np.random.default_rng(3)
    pts = random_cloud(rng, 300, extent=50, lo=-25)[:, 1:]
    v2 = oracle.octree_encode(pts, 32768, version=2)
    v4 = ref4.encode(pts, pts[:77])
    assert G.geometry_info(v2) == {"version": 2, "points": 300, "predicted": False, "reference_points": 0}
    assert G.geometry_info(v4) == {"version": 4, "points": 300, "predicted": True, "reference_points": 77}
    empty = bytes([ord("O"), 2]) + bytes(22)
    assert G.geometry_info(empty) == {"version": 2, "points": 0, "predicted": False, "reference_points": 0}
    for bad in (v4[:-2], v4[:100], v4[:10], b"", v2[:-2], oracle.octree_encode(pts, 32768, version=1)):
        with pytest.raises(PccError):
            G.geometry_info(bad)
    damaged = bytearray(v4)
    damaged[24] ^= 1                  # the root level no longer has one node
    with pytest.raises(PccError):
        G.geometry_info(bytes(damaged))


def test_argument_checks_of_the_new_keywords():
    """raised before anything touches the device"""
    G = _geo_class()
    geo = G.__new__(G)                # no Runtime: the checks come first
    f = [np.zeros((2, 3), np.int16)]
    with pytest.raises(ValueError, match="predict"):
        geo.compress(f, predict="next")
    with pytest.raises(ValueError, match="predict"):
        geo.compress(f, predict=True)
    with pytest.raises(ValueError, match="intra_period"):
        geo.compress(f, intra_period=3)
    with pytest.raises(ValueError, match="reference"):
        geo.compress(f, reference=f[0])
    for bad in (True, 2.0, "3"):
        with pytest.raises(TypeError, match="intra_period"):
            geo.compress(f, predict="previous", intra_period=bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="intra_period"):
            geo.compress(f, predict="previous", intra_period=bad)
    with pytest.raises(ValueError, match="reference"):
        geo.compress(f, predict="previous", reference=np.zeros((2, 3), np.float32))      # another kind than the frames
    with pytest.raises(ValueError, match="reference"):
        geo.compress(f, predict="previous", reference=np.zeros((2, 2), np.int16))
    with pytest.raises((TypeError, ValueError), match="reference"):
        geo.decompress([b""], reference=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="reference"):
        geo.decompress([b""], reference=np.zeros((2, 4), np.int32))
    v4 = ref4.encode(np.array([[1, 2, 3]]), np.array([[1, 2, 3]]))
    with pytest.raises(ValueError, match="frame 1.*version 4.*lod 0"):
        geo.decompress([bytes([ord("O"), 2]) + bytes(22), v4], lod=2, reference=np.zeros((1, 3), np.int32))
