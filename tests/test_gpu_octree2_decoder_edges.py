"""The version-2 decoder kernels (csrc/octree2.hip: k_o2_dec, k_o2_popc, k_o2_link, k_o2_points) on blobs that the
format allows and no encoder of the project writes, through GeometryCodec.decompress(blobs, lod=k), host and device
output, against np.unique of the input and against the reader of octree2_layout_ref.py.  The blobs, their properties
and the damaged ones are built (and asserted, without a GPU) in test_octree2_layouts.py; every test here asserts again
from the blob the property it exists for:
  S at both ends, more than 64 chunks     23 017 nodes at S = 4 (90 chunks: the sum of the chunk table in front of a chunk
                                          takes a second round of the wave; chunks start on a dword and off one), 8, 36, 512
  a layout that is not minimal            2 164 nodes at S = 256 and 512: lanes 9 .. 63 (5 .. 63) code nothing
  the encoder's second chunk              32 768 nodes (S = 512, every lane full) and 32 769 (S = 260, two chunks), through
                                          the GPU encoder, byte for byte
  cuts at lane and chunk edges            every lod 1 .. 15 of S = 4, 8, 36, 512: l* = 63, N' % S == 0, c* = 66, N' = 0 .. 3
                                          mod 4; from the plan's bytes, the whole blob and a prefix in between; one byte
                                          less is refused
  one call over different frames          layouts that differ, a root cube alone, an empty frame, node counts 1, 2, 3
                                          mod 4, in both orders, at lod 0, 3 and 15
  constructed refusals                    status 1 and status 8 each reached by construction, a chunk past the LDS room
  the in-place word route, decoding       a stream at one word per decision: chunks of 181 752 and of about 65 000 words
                                          that decode without a status bit, whole and cut"""
import re

import numpy as np
import pytest

import octree2_layout_ref as ref2
from conftest import pkg
from test_octree2_layouts import (DAMAGED, STATUS_1_ALONE, between, blob, call_frames, check_cuts, cloud, damaged, morton_sorted,
                                  scattered_blob, slow_blob, sparse_blob, switch_frame)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo(rt):
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _decode(geo, blobs, lod=0):
    """the frames of one call, from the device output; the host output of the same call must be the same"""
    dev = geo.decompress(blobs, output="device", lod=lod)
    host = geo.decompress(blobs, lod=lod)
    assert len(dev) == len(host) == len(blobs)
    out = []
    for d, h in zip(dev, host):
        assert d.is_cuda and str(d.dtype) == "torch.int32" and h.dtype == np.int32
        out.append(d.cpu().numpy())
        assert np.array_equal(out[-1], h)
    return out


_done = {}


def _checked(geo, key, b, pts):
    """one blob through the decoder at lod 0, once per module: against the input and against the reader"""
    if key not in _done:
        (got,) = _decode(geo, [b])
        want = morton_sorted(pts)
        assert got.shape == want.shape and np.array_equal(got, want), ref2.header(b)
        assert np.array_equal(ref2.decode(b), want)
        _done[key] = b
    return _done[key]


def _refused(geo, blobs, frame, lod=0):
    """the call is refused with PCC_E_STREAM and names the frame -> the status in the message (None: refused by the
    parser)"""
    abi = pkg("_abi")
    with pytest.raises(abi.PccError) as e:
        geo.decompress(blobs, lod=lod)
    msg = str(e.value)
    assert e.value.code == abi.PCC_E_STREAM, msg
    assert "frame %d:" % frame in msg, msg
    m = re.search(r"status (\d+)", msg)
    return int(m.group(1)) if m else None


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("S", [4, 8, 36, 512])
def test_s_at_both_ends_and_more_than_64_chunks(geo, S):
    b = scattered_blob(S)
    h = ref2.header(b)
    print("scattered: nodes", h["n_nodes"], "S", S, "chunks", h["nc"], "odd word counts", sum(w % 2 for w in h["table"]))
    assert h["nc"] == -(-23017 // (64 * S)) and (S != 4 or h["nc"] == 90 > 64) and (S != 512 or h["nc"] == 1)
    _checked(geo, ("scattered", S), b, cloud("scattered"))


@pytest.mark.parametrize("S", [256, 512])
def test_a_layout_that_is_not_minimal(geo, S):
    b = sparse_blob(S)
    _, lens = ref2.chunk(b, 0)
    assert ref2.header(b)["nc"] == 1 and np.all(lens[-(-2164 // S):] == 0) and np.all(lens[:-(-2164 // S)] > 0)
    _checked(geo, ("seed0", S), b, cloud("seed0"))


def test_an_initial_table_as_given(geo):
    """p0 flat and p0 at the clamps: the decoder takes the table from the blob, not from the counts"""
    for p0 in ([2048] * 108, [16 if i % 2 else 4080 for i in range(108)]):
        b = blob("seed0", 36, p0=tuple(p0))
        assert b != blob("seed0", 36)
        _checked(geo, ("seed0", 36, p0[0]), b, cloud("seed0"))


@pytest.mark.parametrize("delta", [0, 1])
def test_either_side_of_the_encoders_second_chunk(geo, delta):
    """the one place where these tests run k_o2_enc / k_o2_pack: the encoder's bytes are the writer's"""
    pts, b = switch_frame(delta)
    h = ref2.header(b)
    assert h["n_nodes"] == 32768 + delta and (h["S"], h["nc"]) == ((512, 1), (260, 2))[delta]
    (own,) = geo.compress([pts])
    assert own == b, (len(own), len(b), ref2.header(own)["S"])
    _checked(geo, ("switch", delta), own, pts)


# ------------------------------------------------------------------ cuts
@pytest.mark.parametrize("name,S", [("scattered", 4), ("scattered", 8), ("scattered", 36), ("scattered", 512), ("seed18", 4), ("seed40", 4)])
def test_cuts_at_lane_and_chunk_edges(geo, name, S):
    b, pts = check_cuts(name, S), cloud(name)      # check_cuts asserts the table of (N', c*, l*) of this layout
    G = type(geo)
    for k in range(1, 16):
        p = ref2.plan(b, k)
        assert G.lod_info(b, k) == (p["bytes"], p["cells"])
        want = morton_sorted(pts, k)
        assert np.array_equal(ref2.decode(b[:p["bytes"]], k), want), k
        got = _decode(geo, [b[:p["bytes"]], b, b[:between(b, k)]], lod=k)      # one call: the three are frames of it
        for what, g in zip(("the plan's bytes", "the whole blob", "a prefix in between"), got):
            assert g.shape == want.shape and np.array_equal(g, want), (name, S, k, what, p)
        assert _refused(geo, [b[:p["bytes"] - 1]], 0, lod=k) is None, (name, S, k)
    _checked(geo, (name, S), b, pts)      # the codec decodes after the refusals


# ------------------------------------------------------------------ one call over different frames
@pytest.mark.parametrize("lod", [0, 3, 15])
def test_one_call_over_different_frames(geo, lod):
    frames = call_frames()
    blobs = [b for _, _, b in frames]
    single = [_decode(geo, [b], lod)[0] for b in blobs]
    for (label, pts, b), one in zip(frames, single):
        want = morton_sorted(pts, lod).reshape(-1, 3)
        assert one.shape == want.shape and np.array_equal(one, want), (label, lod)
        p = ref2.plan(b, lod)
        if lod == 3 and label in ("one point", "25 nodes", "26 nodes", "27 nodes"):
            assert p["nodes"] == 0 and one.shape[0] == 1      # the root cube alone: no node of this frame is decoded
        if lod == 15 and pts.shape[0] > 1 and ref2.header(b)["depth"] == 16:
            assert p["nodes"] == 1      # a frame of one node between frames of none
    if lod == 0:      # the node ranges of the frames in the call's arrays: padding behind 23 017, 2 164, 25, 26 and 27 nodes
        assert [ref2.plan(b, 0)["nodes"] % 4 for b in blobs] == [1, 1, 0, 0, 1, 1, 2, 3]
    for order in (list(range(len(blobs))), list(range(len(blobs)))[::-1]):
        got = _decode(geo, [blobs[i] for i in order], lod)
        for i, g in zip(order, got):
            assert g.shape == single[i].shape and np.array_equal(g, single[i]), (frames[i][0], lod, order[0])


# ------------------------------------------------------------------ constructed refusals
@pytest.mark.parametrize("name", DAMAGED)
def test_constructed_refusals(geo, name):
    G = type(geo)
    bad, want, good, cname = damaged()[name]
    assert ref2.status(bad) == want and ref2.status(good) == 0
    assert G.geometry_info(bad) == G.geometry_info(good)      # the header's parser has nothing against it
    # (where the nodes behind the damage decode to anything, their counts may be off as well: bit 8 beside bit 1)
    allowed = (want,) if want == 8 or name in STATUS_1_ALONE else (1, 9)
    got = _refused(geo, [bad], 0)
    print(name, "-> status", got)
    assert got in allowed, (name, got)
    other = blob("small881", 8)
    for at in (0, 1, 2):      # in a call of three frames the damaged one is named
        batch = [other, good]
        batch.insert(at, bad)
        assert _refused(geo, batch, at) in allowed, (name, at)
    # the next call on the codec decodes
    (after,) = _decode(geo, [good])
    assert np.array_equal(after, morton_sorted(cloud(cname))), name
    if name == "a bit added in the deepest level":
        # the documented limit of what a prefix can verify: the level sizes below the cut and n itself
        k1 = morton_sorted(cloud(cname), 1)
        for src in (bad, bad[:ref2.plan(bad, 1)["bytes"]]):
            assert np.array_equal(_decode(geo, [src], lod=1)[0], k1)
    if name in ("a bit added in level 11", "a bit moved from level 12 to level 13"):
        assert _refused(geo, [bad], 0, lod=1) == 8      # above the cut of lod 1: verified by the prefix too
        assert np.array_equal(_decode(geo, [bad], lod=5)[0], morton_sorted(cloud(cname), 5))      # below the cut of lod 5


def test_a_chunk_past_the_lds_room_is_refused_in_place(geo):
    """the chunk's table entry and lens announce 24 780 words more than its nodes take, all present: k_o2_dec reads it
    where it lies (word_at clamps every index to the chunk's announced words, which o2_parse has checked against the
    payload, and the payload is uploaded whole) and finds the words of the lanes without nodes unused"""
    bad, want, good, _ = damaged()["24 780 words in the lanes without nodes"]
    h = ref2.header(bad)
    assert h["nc"] == 1 and h["table"][0] > ref2.DEC_LDS_WORDS >= ref2.header(good)["table"][0]
    assert len(bad) == h["off_payload"] + 2 * h["table"][0]
    assert _refused(geo, [bad], 0) == 1
    assert _refused(geo, [good, bad], 1) == 1
    # lod 15 needs lane 0's run alone, 192 + len[0] words of the chunk: the prefix rule does not look at the other lens
    assert np.array_equal(_decode(geo, [bad], lod=15)[0], morton_sorted(cloud("seed0"), 15))


# ------------------------------------------------------------------ the in-place word route on streams that decode
@pytest.mark.parametrize("S", [512, 128])
def test_chunks_past_the_lds_room_that_decode(geo, S):
    """one word per decision (octree2_layout_ref.slow_lane): the chunks are longer than kDecLdsWords and the stream
    leaves no status bit, so IN_LDS = false decodes — whole, and cut where the prefix of the last chunk is longer than
    the room (lod 1) and where it fits (lod 4, the same blob through IN_LDS = true)"""
    b, pts = slow_blob(S), cloud("scattered")
    h = ref2.header(b)
    print("one word per decision: S", S, "chunk words", h["table"], "bytes", len(b))
    assert min(h["table"]) > ref2.DEC_LDS_WORDS
    _checked(geo, ("slow", S), b, pts)
    for k in (1, 4, 9):
        p = ref2.plan(b, k)
        at, _ = ref2.chunk(b, p["c_star"])
        last_words = (p["bytes"] - at) // 2
        if S == 512:
            assert (last_words > ref2.DEC_LDS_WORDS) == (k == 1), (k, last_words)
        want = morton_sorted(pts, k)
        got = _decode(geo, [b[:p["bytes"]], scattered_blob(36), b], lod=k)      # beside a frame of an ordinary stream
        assert all(np.array_equal(g, want) for g in got), (S, k)
