"""Version-2 octree blobs under layouts, cuts and streams that no encoder of the project writes — the host half: the
writer and reader of octree2_layout_ref.py against the existing coders, their round trips at every level of detail,
pcc_octree_lod_info / pcc_octree_inter_info against the restated plan, the bound of the words a chunk can take, and
every property that test_gpu_octree2_decoder_edges.py relies on, asserted here from the blobs so that a changed seed
fails without a GPU first.  The builders below (clouds, blobs, cuts, damaged blobs) are the GPU file's too."""
import math
import struct

import numpy as np
import pytest

import octree2_layout_ref as ref2
import octree_inter_ref as ref4
from conftest import pkg
from test_octree2 import _clouds, py_octree2_encode
from test_octree_inter_gpu import _boundary_cloud

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ clouds and what a decode of them gives
def morton_sorted(p, k=0):
    """the distinct cells p >> k in Morton order, int32 [m, 3]: what a decode at level of detail k returns"""
    c = np.unique(np.asarray(p, np.int32).reshape(-1, 3) >> k, axis=0)
    return c[np.argsort(ref4.morton(c.astype(np.int64) + (32768 >> k)), kind="stable")]


SCATTERED_LEVELS = [1] + [8] * 8 + [64, 216, 998, 4071, 5663, 5947, 5993]
# prefixes of one shuffled dense cloud, found by bisection on the CPU with octree_inter_ref.build_tree: the longest with
# 32 768 nodes (the encoder's one chunk of S = 512, every lane full) and the next (two chunks of S = 260)
SWITCH_POINTS = 56465
# np.unique(default_rng(seed).integers(0, 8, (20, 3))): depth 3 and 25 / 26 / 27 nodes, 1 / 2 / 3 mod 4
TINY_SEEDS = {1: 0, 2: 5, 3: 2}


def cloud(name):
    def make():
        if name == "scattered":      # 5 999 points, depth 16, 23 017 nodes
            return np.unique(np.random.default_rng(3).integers(-150, 150, (6000, 3)), axis=0).astype(np.int32)
        if name.startswith("seed"):      # about 2 200 nodes, depth 16
            return _boundary_cloud(int(name[4:]))
        if name == "small881":
            return _boundary_cloud(0)[:160]
        if name == "dense":
            rng = np.random.default_rng(1)
            pts = np.unique(rng.integers(0, 64, (90000, 3)), axis=0).astype(np.int32)
            return pts[rng.permutation(len(pts))]
        if name.startswith("tiny"):
            return np.unique(np.random.default_rng(TINY_SEEDS[int(name[4:])]).integers(0, 8, (20, 3)), axis=0).astype(np.int32)
        if name == "one point":
            return np.array([[-7, 300, 12]], np.int32)
        if name == "empty":
            return np.zeros((0, 3), np.int32)
        raise KeyError(name)
    return cached(("cloud", name), make)


def blob(name, S=None, **kw):
    """the writer's blob of a cloud under a layout, once per session"""
    return cached(("blob", name, S, tuple(sorted(kw.items(), key=lambda kv: kv[0]))), lambda: ref2.encode(cloud(name), S=S, **kw))


# the forced layouts of both files: (cloud, S)
LAYOUTS = [("scattered", 4), ("scattered", 8), ("scattered", 36), ("scattered", 512), ("seed0", 256), ("seed0", 512),
           ("seed18", 4), ("seed40", 4), ("small881", 8), ("tiny1", 4), ("tiny2", 8), ("tiny3", 512)]


# ------------------------------------------------------------------ the blobs of the GPU file, each with its property
def scattered_blob(S):
    """S at both ends: 90 chunks at S = 4 (more than the 64 a wave sums of the chunk table in one round; 40 of them with
    an odd word count, so chunks start both on a dword and off one), 45 at S = 8, 10 at S = 36, 1 at S = 512"""
    b = blob("scattered", S)
    h = ref2.header(b)
    assert (h["n"], h["depth"], h["n_nodes"], h["level_n"]) == (5999, 16, 23017, SCATTERED_LEVELS)
    assert h["S"] == S and h["nc"] == {4: 90, 8: 45, 36: 10, 512: 1}[S]
    if S == 4:
        odd = [w % 2 for w in h["table"]]
        assert sum(odd) == 40
        starts = np.cumsum([0] + h["table"][:-1]) % 2
        assert 0 < starts.sum() < 90 and starts[64:].any() and not starts[64:].all()      # both kinds behind chunk 64 too
    return b


def sparse_blob(S):
    """a layout that is not minimal: 2 164 nodes dealt 256 (512) to a lane: one chunk, lanes 9 .. 63 (5 .. 63) hold no
    node and have len == 0"""
    b = blob("seed0", S)
    h = ref2.header(b)
    first_empty = {256: 9, 512: 5}[S]
    assert h["n_nodes"] == 2164 and h["nc"] == 1 and -(-2164 // S) == first_empty
    _, lens = ref2.chunk(b, 0)
    assert np.all(lens[first_empty:] == 0) and np.all(lens[:first_empty] > 0)
    return b


def switch_frame(delta):
    """either side of the encoder's second chunk: (points, the writer's blob in the ENCODER's layout)"""
    pts = cloud("dense")[:SWITCH_POINTS + delta]
    b = cached(("switch", delta), lambda: ref2.encode(pts))
    h = ref2.header(b)
    assert h["depth"] == 6 and h["n_nodes"] == 32768 + delta and (h["S"], h["nc"]) == ((512, 1), (260, 2))[delta]
    _, lens = ref2.chunk(b, h["nc"] - 1)
    if delta:      # chunk 1: 16 129 nodes, 62 lanes of 260 and one of 9; lane 63 holds none
        assert 32769 - 64 * 260 == 62 * 260 + 9 and np.all(lens[:63] > 0) and lens[63] == 0
    else:
        assert np.all(lens > 0)
    return pts, b


# (cloud, S, lod) -> (N', c*, l*): the cuts at lane and chunk edges; N' % S == 0 means no lane straddles the cut
CUTS = {("scattered", 4, 1): (17024, 66, 31), ("scattered", 4, 2): (11077, 43, 17), ("scattered", 4, 3): (5414, 21, 9),
        ("scattered", 4, 4): (1343, 5, 15), ("scattered", 8, 1): (17024, 33, 15), ("scattered", 36, 1): (17024, 7, 24),
        ("scattered", 512, 1): (17024, 0, 33), ("scattered", 512, 4): (1343, 0, 2), ("scattered", 512, 5): (345, 0, 0),
        ("seed18", 4, 5): (256, 0, 63), ("seed40", 4, 1): (1792, 6, 63)}


def check_cuts(name, S):
    """the plan of every lod of a layout against CUTS and against the rule's own arithmetic"""
    b = blob(name, S)
    h = ref2.header(b)
    for k in range(1, 16):
        p = ref2.plan(b, k)
        want = CUTS.get((name, S, k))
        if want:
            assert (p["nodes"], p["c_star"], p["l_star"]) == want, (name, S, k, p)
        if p["nodes"]:
            assert p["lanes"] == -(-p["nodes"] // S) and 64 * p["c_star"] + p["l_star"] + 1 == p["lanes"]
        assert p["cells"] == len(morton_sorted(cloud(name), k))
    if (name, S) == ("scattered", 4):      # lod 1: c* >= 64 and no straddling lane; lods 2, 3, 4: N' = 1, 2, 3 mod 4
        assert ref2.plan(b, 1)["c_star"] >= 64 and ref2.plan(b, 1)["nodes"] % S == 0
        assert [ref2.plan(b, k)["nodes"] % 4 for k in (2, 3, 4)] == [1, 2, 3]
    if (name, S) == ("scattered", 8):
        assert ref2.plan(b, 1)["nodes"] % S == 0
    if (name, S) == ("scattered", 512):      # every cut inside chunk 0, with a straddling lane
        assert all(ref2.plan(b, k)["c_star"] == 0 and ref2.plan(b, k)["nodes"] % S for k in range(1, 16))
    if (name, S) in (("seed18", 4), ("seed40", 4)):      # lanes_last = 64 on a cut tree: the cut lies on a chunk boundary
        k = 5 if name == "seed18" else 1
        assert ref2.plan(b, k)["nodes"] % (64 * S) == 0 and ref2.plan(b, k)["nodes"] < h["n_nodes"]
    return b


def between(b, k):
    """a prefix length strictly between the plan's bytes and the whole blob (odd, so it ends inside a word)"""
    need = ref2.plan(b, k)["bytes"]
    assert need + 2 < len(b)
    return (need + len(b)) // 2 | 1


def call_frames():
    """one call over different frames: [(label, points, blob)] — layouts that differ, frames without a node to decode
    (one point: its root cube at every lod >= 1; empty), node counts 1, 2, 3 mod 4 (padding between the frames' node
    ranges), the encoder's own layout beside a forced one of the same cloud"""
    out = [("scattered S=4", "scattered", 4), ("one point", "one point", None), ("empty", "empty", None), ("seed0 S=512", "seed0", 512),
           ("scattered, the encoder's layout", "scattered", None), ("25 nodes", "tiny1", 4), ("26 nodes", "tiny2", 8),
           ("27 nodes", "tiny3", 512)]
    frames = [(label, cloud(name), blob(name, S)) for label, name, S in out]
    assert len(frames[2][2]) == 24 and ref2.header(frames[1][2])["depth"] == 1
    assert [ref2.header(f[2])["n_nodes"] % 4 for f in frames[5:]] == [1, 2, 3]
    assert all(ref2.header(f[2])["depth"] == 3 for f in frames[5:])      # root cubes alone from lod 3 on
    own = ref2.header(frames[4][2])
    assert (own["S"], own["nc"]) == (360, 1)
    return frames


# ------------------------------------------------------------------ damaged blobs, the status known in advance
def resize_lane(b, c, l, delta, fill=0):
    """lane l of chunk c with `delta` words more (of value fill, behind its run) or fewer (off its end): its len, the
    chunk's table entry and the payload length follow, so the parser has nothing against the blob"""
    h = ref2.header(b)
    at, lens = ref2.chunk(b, c)
    end = at + 2 * (192 + int(lens[:l + 1].sum()))
    out = bytearray(b)
    if delta >= 0:
        out[end:end] = struct.pack("<%dH" % delta, *[fill] * delta)
    else:
        assert lens[l] >= -delta
        del out[end + 2 * delta:end]
    struct.pack_into("<H", out, at + 2 * (128 + l), int(lens[l]) + delta)
    struct.pack_into("<I", out, h["off_table"] + 4 * c, h["table"][c] + delta)
    struct.pack_into("<I", out, 20, len(out) - 24)
    return bytes(out)


def another_s(b, S):
    """another S in the header that the parser accepts: every node is dealt to another lane"""
    h = ref2.header(b)
    assert S != h["S"] and S % 4 == 0 and 64 * S * (h["nc"] - 1) < h["n_nodes"] <= 64 * S * h["nc"]
    out = bytearray(b)
    struct.pack_into("<I", out, 24 + 4 * h["depth"], S)
    return bytes(out)


def _tree_bytes(name):
    levels, _, depth, org, n = ref4.build_tree(cloud(name))
    return [list(lv) for lv in levels], n, [int(v) - 32768 for v in org]


def _add_bit(byte):
    free = [j for j in range(8) if not (byte >> j) & 1]
    return byte | (1 << free[0])


# the names of damaged()'s blobs (pytest needs them before the blobs are made), and those whose status is 1 and nothing
# else: every node of theirs decodes as in the good blob, so no count can be off
DAMAGED = ["a lane without nodes announces a word", "a run one word short", "192 + sum(len) against the table entry",
           "the last len of chunk 26 of 45 one less", "S = 512 rewritten to 360", "S = 512 rewritten to 508", "S = 8 rewritten to 12",
           "a bit added in level 11", "a bit moved from level 12 to level 13", "a bit added in the deepest level",
           "the bytes of a tree of levels 1, 3, 3 under a header of 1, 2, 4", "24 780 words in the lanes without nodes",
           "a run one word short, read in place", "a run one word long, read in place"]
STATUS_1_ALONE = ["a lane without nodes announces a word", "24 780 words in the lanes without nodes",
                  "a run one word short, read in place", "a run one word long, read in place"]


def damaged():
    """name -> (damaged blob, status the kernels must report, the good blob it was made from, its cloud's name).
    Status 1: k_o2_dec (words); 8 alone: k_o2_link (counts), from streams whose every word is consumed."""
    def make():
        out = {}
        sp = sparse_blob(256)
        out["a lane without nodes announces a word"] = (resize_lane(sp, 0, 63, 1, 0x1234), 1, sp, "seed0")
        out["a run one word short"] = (resize_lane(sp, 0, 3, -1), 1, sp, "seed0")
        at, lens = ref2.chunk(sp, 0)
        longer = bytearray(sp)      # len[5] + 1, the table entry left as it is
        struct.pack_into("<H", longer, at + 2 * (128 + 5), int(lens[5]) + 1)
        out["192 + sum(len) against the table entry"] = (bytes(longer), 1, sp, "seed0")
        s8 = scattered_blob(8)
        at, lens = ref2.chunk(s8, 26)      # a chunk in the middle of 45
        shorter = bytearray(s8)
        struct.pack_into("<H", shorter, at + 2 * (128 + 63), int(lens[63]) - 1)
        out["the last len of chunk 26 of 45 one less"] = (bytes(shorter), 1, s8, "scattered")
        # (the 45 chunks of S = 8 and the 90 of S = 4 of the scattered frame admit no other S; its one chunk of S = 512
        # admits 360 .. 508)
        s512 = scattered_blob(512)
        for S in (360, 508):
            out["S = 512 rewritten to %d" % S] = (another_s(s512, S), 1, s512, "scattered")
        small = blob("small881", 8)
        assert ref2.header(small)["n_nodes"] == 881 and ref2.header(small)["nc"] == 2
        out["S = 8 rewritten to 12"] = (another_s(small, 12), 1, small, "small881")

        # status 8 alone: the bytes as given, every word consumed
        levels, n, org = _tree_bytes("scattered")
        good = scattered_blob(36)
        lv = [list(x) for x in levels]
        lv[11][500] = _add_bit(lv[11][500])
        out["a bit added in level 11"] = (ref2.encode_bytes(lv, n, org, 36), 8, good, "scattered")
        lv = [list(x) for x in levels]
        a = next(i for i, v in enumerate(lv[12]) if bin(v).count("1") >= 2)
        lv[12][a] &= lv[12][a] - 1      # its lowest bit goes ..
        # .. to a node of the next level: the total is kept.  (Level 13 then begins one node early, and the leaves under
        # the node that moved down a level walk 17 links: k_o2_link's per-level check AND k_o2_points see it.  What the
        # per-level check alone sees is the tree below, of other level sizes.)
        lv[13][2000] = _add_bit(lv[13][2000])
        out["a bit moved from level 12 to level 13"] = (ref2.encode_bytes(lv, n, org, 36), 8, good, "scattered")
        lv = [list(x) for x in levels]
        lv[15][3000] = _add_bit(lv[15][3000])
        out["a bit added in the deepest level"] = (ref2.encode_bytes(lv, n, org, 36), 8, good, "scattered")
        # another tree under this header: depth 3, level sizes 1, 3, 3 and 5 points coded where the header announces
        # 1, 2, 4 and 5 points — 7 nodes, 11 children and every leaf at depth 3 in both, so neither the total nor the
        # leaves' walks (k_o2_points) can tell them apart: level 2 begins at node 4, not at node 3
        t1 = np.array([[0, 0, 0], [0, 0, 1], [0, 2, 0], [4, 0, 0], [4, 2, 0]], np.int32)      # 1, 2, 4
        t2 = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 4, 0], [4, 0, 0]], np.int32)      # 1, 3, 3
        l1, l2 = ref4.build_tree(t1)[0], ref4.build_tree(t2)[0]
        assert [len(x) for x in l1] == [1, 2, 4] and [len(x) for x in l2] == [1, 3, 3]
        assert sum(bin(v).count("1") for x in l1 for v in x) == sum(bin(v).count("1") for x in l2 for v in x) == 11
        _cache[("cloud", "tree 1 2 4")] = t1
        alien = ref2.encode_bytes([v for x in l2 for v in x], 5, [0, 0, 0], 4, level_n=[1, 2, 4])
        out["the bytes of a tree of levels 1, 3, 3 under a header of 1, 2, 4"] = (alien, 8, ref2.encode(t1, S=4), "tree 1 2 4")

        # a chunk past the LDS room, refused: the lens of the lanes without nodes and the table entry announce more than
        # kDecLdsWords words, and the words (zeros) are there
        sp5 = sparse_blob(512)
        big = sp5
        for l in range(5, 64):
            big = resize_lane(big, 0, l, 420)
        assert ref2.header(big)["table"][0] > ref2.DEC_LDS_WORDS and ref2.header(sp5)["table"][0] + 59 * 420 == ref2.header(big)["table"][0]
        out["24 780 words in the lanes without nodes"] = (big, 1, sp5, "seed0")
        slow = slow_blob(512)
        out["a run one word short, read in place"] = (resize_lane(slow, 0, 30, -1), 1, slow, "scattered")
        out["a run one word long, read in place"] = (resize_lane(slow, 0, 30, 1), 1, slow, "scattered")
        return out
    return cached("damaged", make)


def slow_blob(S):
    """the scattered frame at one word per decision (octree2_layout_ref.slow_lane): a stream that every decoder reads
    without complaint and whose chunks are longer than kDecLdsWords: S = 512, one chunk of 181 752 words; S = 128, three
    chunks, the first two of 64 x 128 nodes each"""
    b = blob("scattered", S, lane=ref2.slow_lane)
    h = ref2.header(b)
    assert h["nc"] == {512: 1, 128: 3}[S] and min(h["table"]) > ref2.DEC_LDS_WORDS, h["table"]
    if S == 512:
        assert h["table"] == [181752]
    return b


# ------------------------------------------------------------------ the writer against the existing coders
@pytest.mark.parametrize("name", [n for n, _ in _clouds()] + ["scattered"])
def test_the_writer_in_the_encoders_layout(oracle, name):
    pts = (cloud("scattered") if name == "scattered" else dict(_clouds())[name]).astype(np.int32)
    b = ref2.encode(pts)
    assert b == py_octree2_encode(pts, 32768)
    assert b == oracle.octree_encode(pts, 32768, version=2)
    assert np.array_equal(ref2.decode(b), morton_sorted(pts))
    assert ref2.encode(np.zeros((0, 3), np.int32)) == oracle.octree_encode(np.zeros((0, 3), np.int32), 32768, version=2)


@pytest.mark.parametrize("name,S", LAYOUTS)
def test_forced_layouts_round_trip(oracle, name, S):
    """the reader inverts the writer at lod 0 and at every cut; the oracle's decoder, which takes any S, reads the blob
    too; from the plan's bytes, from the whole blob and from a prefix in between"""
    b, pts = blob(name, S), cloud(name)
    h = ref2.header(b)
    assert h["S"] == S and h["nc"] == max(1, -(-h["n_nodes"] // (64 * S)))
    assert np.array_equal(ref2.decode(b), morton_sorted(pts))
    assert np.array_equal(oracle.octree_decode(b), morton_sorted(pts))
    for k in range(1, 16):
        want = morton_sorted(pts, k)
        need = ref2.plan(b, k)["bytes"]
        assert np.array_equal(ref2.decode(b[:need], k), want), (name, S, k)
        assert np.array_equal(ref2.decode(b, k), want), (name, S, k)
        if need + 2 < len(b):
            assert np.array_equal(ref2.decode(b[:between(b, k)], k), want), (name, S, k)
        with pytest.raises(ValueError, match="truncated"):
            ref2.decode(b[:need - 1], k)


@pytest.mark.parametrize("table", ["flat", "extremes"])
def test_an_initial_table_as_given(oracle, table):
    """p0 is part of the format, not of the encoder: any probabilities in 16 .. 4080"""
    p0 = [2048] * 108 if table == "flat" else [16 if i % 2 else 4080 for i in range(108)]
    b = blob("seed0", 36, p0=tuple(p0))
    assert list(struct.unpack_from("<108H", b, ref2.header(b)["off_p0"])) == p0 and b != blob("seed0", 36)
    assert np.array_equal(ref2.decode(b), morton_sorted(cloud("seed0")))
    assert np.array_equal(oracle.octree_decode(b), morton_sorted(cloud("seed0")))
    for bad in ([15] + [2048] * 107, [2048] * 107):
        with pytest.raises(ValueError):
            ref2.encode(cloud("seed0"), S=36, p0=bad)


# ------------------------------------------------------------------ the host entry points against the plan
@pytest.mark.parametrize("name,S", LAYOUTS)
def test_lod_info_and_geometry_info_against_the_plan(name, S):
    abi = pkg("_abi")
    G = pkg().GeometryCodec
    b = check_cuts(name, S) if any(key[:2] == (name, S) for key in CUTS) else blob(name, S)
    h = ref2.header(b)
    assert G.geometry_info(b) == {"version": 2, "points": h["n"], "predicted": False, "reference_points": 0}
    for k in range(16):
        p = ref2.plan(b, k)
        assert G.lod_info(b, k) == (p["bytes"], p["cells"]), (name, S, k)
        assert G.lod_info(b[:p["bytes"]], k) == (p["bytes"], p["cells"]), (name, S, k)
        if k and p["nodes"]:      # one byte inside the last needed length table: refused; the table whole: answered
            at, _ = ref2.chunk(b, p["c_star"])
            assert G.lod_info(b[:at + 2 * 192], k) == (p["bytes"], p["cells"]), (name, S, k)
            with pytest.raises(abi.PccError) as e:
                G.lod_info(b[:at + 2 * 192 - 1], k)
            assert e.value.code == abi.PCC_E_STREAM, (name, S, k)
    if (name, S) == ("scattered", 4):
        assert ref2.plan(b, 1)["c_star"] == 66      # lod_info sums 66 table entries in front of the needed chunk


# ------------------------------------------------------------------ properties the GPU file relies on
@pytest.mark.parametrize("S", [4, 8, 36, 512])
def test_scattered_layouts(S):
    scattered_blob(S)
    check_cuts("scattered", S)


@pytest.mark.parametrize("S", [256, 512])
def test_layouts_that_are_not_minimal(S):
    sparse_blob(S)


@pytest.mark.parametrize("name", ["seed18", "seed40"])
def test_cuts_on_a_chunk_boundary(name):
    check_cuts(name, 4)


@pytest.mark.parametrize("delta", [0, 1])
def test_either_side_of_the_encoders_second_chunk(oracle, delta):
    pts, b = switch_frame(delta)
    assert b == oracle.octree_encode(pts, 32768, version=2)
    assert np.array_equal(ref2.decode(b), morton_sorted(pts))


def test_the_frames_of_one_call():
    for label, pts, b in call_frames():
        for k in (0, 3, 15):
            assert np.array_equal(ref2.decode(b, k), morton_sorted(pts, k).reshape(-1, 3)), (label, k)
        if label in ("one point", "25 nodes", "26 nodes", "27 nodes"):
            assert ref2.plan(b, 3)["nodes"] == 0 and ref2.plan(b, 3)["cells"] == 1      # the root cube alone
        if pts.shape[0] > 1:
            assert ref2.plan(b, 0)["nodes"] > 0


def test_damaged_blobs_have_the_status_they_are_built_for(oracle):
    G = pkg().GeometryCodec
    assert list(damaged()) == DAMAGED and all(damaged()[name][1] == 1 for name in STATUS_1_ALONE)
    for name, (bad, status, good, cname) in damaged().items():
        assert G.geometry_info(bad) == G.geometry_info(good), name      # the parser has nothing against it
        assert ref2.status(good) == 0 and ref2.status(bad) == status, name
        with pytest.raises(AssertionError):      # the oracle's decoder refuses it too
            oracle.octree_decode(bad)
    # what a prefix cannot verify: the blob whose deepest level has a child too many decodes at lod 1
    bad = damaged()["a bit added in the deepest level"][0]
    assert np.array_equal(ref2.decode(bad, 1), morton_sorted(cloud("scattered"), 1))
    assert np.array_equal(ref2.decode(bad[:ref2.plan(bad, 1)["bytes"]], 1), morton_sorted(cloud("scattered"), 1))
    # .. while a level above the cut is verified by the prefix too
    for name in ("a bit added in level 11", "a bit moved from level 12 to level 13"):
        assert ref2.status(damaged()[name][0], 1) == 8 and ref2.status(damaged()[name][0], 5) == 0, name


# ------------------------------------------------------------------ the words a chunk can take
def _worst_bits(slack):
    """W[t]: the most bits t decisions in ONE context can cost under o2_adapt from any initial probability 16 .. 4080,
    every decision charged log2(4096 / freq) + slack: a dynamic programme over the 12-bit probability"""
    p = np.arange(4096)
    up, dn = p + ((4096 - p) >> 4), p - (p >> 4)
    live = (p >= 15) & (p <= 4081)      # what adaptation reaches from 16 .. 4080 (asserted below)
    c0 = np.where(live, np.log2(4096.0 / np.maximum(4096 - p, 1)), 0.0) + slack
    c1 = np.where(live, np.log2(4096.0 / np.maximum(p, 1)), 0.0) + slack
    reach = np.zeros(4096, bool)
    reach[16:4081] = True
    for _ in range(4096):
        nxt = reach.copy()
        nxt[up[reach]] = True
        nxt[dn[reach]] = True
        if np.array_equal(nxt, reach):
            break
        reach = nxt
    assert np.array_equal(np.nonzero(reach)[0][[0, -1]], [15, 4081])
    V, W = np.zeros(4096), [0.0]
    for _ in range(512):
        V = np.maximum(c0 + V[dn], c1 + V[up])
        W.append(float(V[16:4081].max()))
    return np.array(W)


def _lane_bound(W, nodes):
    """the most bits `nodes` nodes of ONE level class can cost a lane: bit position j is decided once per node in one
    of its j + 1 contexts (7 at j = 7, whose context `no ones` is implied); the split of the nodes over the contexts
    of a position is the adversary's (a knapsack, no concavity assumed), the positions are independent"""
    total = 0.0
    for j in range(8):
        best = np.full(nodes + 1, -np.inf)
        best[0] = 0.0
        for _ in range(j + 1 if j < 7 else 7):
            nxt = np.full(nodes + 1, -np.inf)
            for t in range(nodes + 1):      # t decisions to this context
                nxt[t:] = np.maximum(nxt[t:], best[:nodes + 1 - t] + W[t])
            best = nxt
        total += best.max()
    return total


def test_the_words_a_chunk_can_take():
    """Can the in-place word route of k_o2_dec (a chunk of more than 24 576 words) be reached by a stream that decodes
    without a status bit?

    For streams of a rANS ENCODER it cannot.  Such a lane's state stays in [2^16, 2^32); a decision of frequency f takes
    the state x to f (x >> 12) + r >= x (f / 4096) (15 / 16), a refill multiplies it by at least 2^16, so the w words a
    lane consumes satisfy 16 w < 32 - 16 + sum (log2(4096 / f) + log2(16 / 15)).  The sum is bounded by the dynamic
    programme above over the model's states (clamps included: adaptation keeps a probability in 15 .. 4081) and a
    knapsack over the contexts of a bit position, per level class; a lane's 512 nodes split over the classes it sees,
    and of the 64 lanes of a chunk at most two see more than one class (the two class boundaries).

    For streams as such it can: no parser looks at a lane's initial state, and from a state below 2^12 a stream can
    spend one word on every decision (octree2_layout_ref.slow_lane).  slow_blob builds one, 181 752 words in a chunk,
    and the reader here, the oracle's decoder and (test_gpu_octree2_decoder_edges.py) the kernels decode it."""
    W = _worst_bits(math.log2(16 / 15))
    plain = _worst_bits(0.0)
    print("worst bits of a context met 38 / 57 / 114 / 512 times: %.1f / %.1f / %.1f / %.1f (%.1f / %.1f / %.1f / %.1f without the "
          "truncation's share)" % tuple(list(W[[38, 57, 114, 512]]) + list(plain[[38, 57, 114, 512]])))
    one = cached("lane bounds", lambda: [_lane_bound(W, m) for m in range(0, 513, 32)])      # one class, 0, 32, .. 512 nodes
    # the classes of a lane: 512 nodes over 1, 2 or 3 classes, in steps of 32 nodes rounded UP (m nodes cost at most
    # what the next multiple of 32 costs: W is monotone)
    def lane_words(bits):
        return int((16 + bits) // 16)
    L1 = lane_words(one[16])
    L2 = lane_words(max(one[a] + one[min(16, 17 - a)] for a in range(17)))
    L3 = lane_words(max(one[a] + one[b] + one[min(16, 18 - a - b)] for a in range(17) for b in range(17 - a)))
    assert all(x <= y + 1e-9 for x, y in zip(one, one[1:]))
    chunk_words = 192 + 62 * L1 + max(2 * L2, L1 + L3)
    print("words of a lane that sees 1 / 2 / 3 level classes: at most %d / %d / %d; of a chunk: %d (kDecLdsWords = %d)"
          % (L1, L2, L3, chunk_words, ref2.DEC_LDS_WORDS))
    assert chunk_words < ref2.DEC_LDS_WORDS
    # the counterexample
    b = slow_blob(512)
    assert ref2.header(b)["table"][0] == 181752 > ref2.DEC_LDS_WORDS
    at, lens = ref2.chunk(b, 0)
    states = struct.unpack_from("<128H", b, at)
    assert all(states[2 * l + 1] == 0 and states[2 * l] < 4096 for l in range(45))      # the lanes with nodes start below 2^12


def test_the_slow_stream_decodes(oracle):
    pts = cloud("scattered")
    for S in (512, 128):
        b = slow_blob(S)
        assert np.array_equal(ref2.decode(b), morton_sorted(pts))
        assert np.array_equal(oracle.octree_decode(b), morton_sorted(pts))
    b = slow_blob(512)
    for k in (1, 4, 9):      # lod 1: 34 lanes, 136 k words, read in place; lod 4: 3 lanes, inside the LDS room
        p = ref2.plan(b, k)
        words = (p["bytes"] - ref2.header(b)["off_payload"]) // 2
        assert (words > ref2.DEC_LDS_WORDS) == (k == 1), (k, words)
        assert np.array_equal(ref2.decode(b[:p["bytes"]], k), morton_sorted(pts, k))
