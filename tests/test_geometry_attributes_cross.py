"""Cross-channel attribute blobs, versions 8, 11, 13 and 14 (include/pcc.h has the rule), on the host: the numpy
restatement tests/attr_cross_ref.py against the restatements of the plain kinds, one blob worked by hand, the size
condition on recorded camera frames, and the host-only entry points (pcc_attr_info, pcc_attr_cross_mask,
pcc_attr_lod_info) with what they refuse.  No GPU."""
import os
import struct

import numpy as np
import pytest

import attr2_ref
import attr_cross_ref
import attr_nl_ref
import attr_ref
from conftest import ROOT, pkg, random_cloud
from test_geometry_attributes_lod import _morton

KINDS = {8: (False, 0), 11: (True, 0), 13: (False, 2), 14: (True, 2)}      # version: (scalable, e of the tests)
MASKS = {2: (True, (1,)), 3: (True, (1,), (2,)), 4: (True, (3,), (1, 2))}      # all, single, (1, 2) of 4


def _correlated(rng, n, c, bpv):
    """c channels that follow one signal, as a camera's colour does, over the whole value range"""
    top = 1 << (8 * bpv)
    base = np.cumsum(rng.integers(-9, 10, n)) * (1 if bpv == 1 else 97) + rng.integers(0, top)
    return ((base[:, None] + rng.integers(-4, 5, (n, c)) * (1 if bpv == 1 else 50)) % top).astype(np.int64)


def _encode(vals, bpv, cross, ver, pts, e=None):
    scalable, e0 = KINDS[ver]
    e = e0 if e is None else e
    return attr_cross_ref.encode(vals, bpv, cross, e, points=pts if scalable else None)


def _plain(vals, bpv, ver, pts, e=None):
    scalable, e0 = KINDS[ver]
    return attr_nl_ref.encode(vals, bpv, e0 if e is None else e, points=pts if scalable else None)


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(77)
    out = {}
    for n in (1, 2, 65, 300):
        pts = random_cloud(rng, n, extent=60, lo=-30)[:, 1:]
        out[n] = pts[np.argsort(attr2_ref.keys_of(pts))]                     # Morton order: row i of the values is point i
    return out


@pytest.mark.parametrize("ver", sorted(KINDS))
@pytest.mark.parametrize("bpv", [1, 2])
@pytest.mark.parametrize("c", [2, 3, 4])
def test_round_trip_and_equality_with_the_plain_kind(clouds, ver, bpv, c):
    """decode(encode(v)) is what the plain kind of the same input decodes to (v itself for the lossless kinds), for every
    mask, at lod 0 and from the prefixes of two coarser levels"""
    rng = np.random.default_rng(1000 * ver + 10 * bpv + c)
    scalable, e = KINDS[ver]
    for n, pts in clouds.items():
        vals = _correlated(rng, n, c, bpv)
        plain = _plain(vals, bpv, ver, pts)
        want = attr_nl_ref.decode(plain, *([pts] if scalable else []))[0]
        assert e or np.array_equal(want, vals)
        for cross in MASKS[c]:
            blob = _encode(vals, bpv, cross, ver, pts)
            m = attr_cross_ref.mask_of(cross, c)
            assert blob[:4] == bytes([ord("A"), ver, plain[2], c | (m << 4)]) and blob[4:8] == plain[4:8], (n, cross)
            got, gb = attr_cross_ref.decode(blob, *([pts] if scalable else []))
            assert gb == bpv and np.array_equal(got, want), (n, cross)
            assert np.abs(got - vals).max() <= e, (n, cross)
            if not scalable or n < 65:
                continue
            for k in (1, 3):
                cells = np.unique(pts >> k, axis=0)
                nb, cnt = attr_cross_ref.lod_info(blob, k)
                pb, pcnt = attr_nl_ref.lod_info(plain, k)
                assert cnt == pcnt == cells.shape[0] and nb <= len(blob), (n, cross, k)
                assert np.array_equal(attr_cross_ref.decode(blob[:nb], cells, k)[0], attr_nl_ref.decode(plain[:pb], cells, k)[0]), (n, cross, k)
                with pytest.raises(AssertionError):
                    attr_cross_ref.decode(blob[:nb - 2], cells, k)


@pytest.mark.parametrize("bpv", [1, 2])
def test_the_largest_max_error_and_e_1(clouds, bpv):
    """the near-lossless kinds at the ends of e: 1, and 2^(8 bpv - 1) - 1, where an index is -1, 0 or 1"""
    rng = np.random.default_rng(5 + bpv)
    pts = clouds[300]
    vals = rng.integers(0, 1 << (8 * bpv), (300, 3))
    for e in (1, (1 << (8 * bpv - 1)) - 1):
        for ver in (13, 14):
            args = [pts] if ver == 14 else []
            blob = _encode(vals, bpv, True, ver, pts, e)
            want = attr_nl_ref.decode(_plain(vals, bpv, ver, pts, e), *args)[0]
            got = attr_cross_ref.decode(blob, *args)[0]
            assert attr_cross_ref.info(blob)["max_error"] == e and np.array_equal(got, want), (e, ver)
            assert np.abs(got - vals).max() <= e, (e, ver)


def test_an_empty_mask_and_one_channel_give_the_plain_blob(clouds):
    pts = clouds[65]
    rng = np.random.default_rng(3)
    for ver in KINDS:
        one = rng.integers(0, 256, (65, 1))
        assert _encode(one, 1, True, ver, pts) == _plain(one, 1, ver, pts)
        three = rng.integers(0, 256, (65, 3))
        assert _encode(three, 1, (), ver, pts) == _encode(three, 1, False, ver, pts) == _plain(three, 1, ver, pts)
        empty = _encode(np.zeros((0, 3), np.int64), 2, (2,), ver, np.zeros((0, 3), np.int64))
        assert empty == bytes([ord("A"), ver, 2, 3 | (2 << 4)]) + bytes(8)
        assert attr_cross_ref.decode(empty, *([np.zeros((0, 3))] if KINDS[ver][0] else []))[0].shape == (0, 3)


@pytest.mark.parametrize("bpv", [1, 2])
@pytest.mark.parametrize("pair", ["ends", "middle"])
def test_differences_wrap_to_the_value_width(clouds, bpv, pair):
    """channels alternating 0 / 255 (0 / 65535), whose unwrapped residuals differ by up to twice the value range; and
    alternating 127 / 128 (32767 / 32768), the two values whose wrapped residuals at a run's start are h - 1 and -h, so
    that w[ch] - w[ch - 1] itself leaves [-h, h) in both directions and must wrap"""
    top = (1 << (8 * bpv)) - 1
    h = (top + 1) // 2
    lo, hi = (0, top) if pair == "ends" else (h - 1, h)
    n = 65
    pts = clouds[n]
    vals = np.full((n, 4), lo, np.int64)
    vals[::2, 0::2] = hi
    vals[1::2, 1::2] = hi
    w = attr_ref._resid(attr_cross_ref._runs(vals, n, 4), bpv)[0].reshape(-1, 4)[:n]
    d = w[:, 1:] - w[:, :-1]
    assert pair == "ends" or ((d >= h).any() and (d < -h).any())
    x = attr_cross_ref.forward(w, 7, bpv)
    assert x.min() >= -h and x.max() < h and np.array_equal(attr_cross_ref.inverse(x, 7, bpv), w)
    for ver in KINDS:
        args = [pts] if KINDS[ver][0] else []
        got = attr_cross_ref.decode(_encode(vals, bpv, True, ver, pts), *args)[0]
        assert np.array_equal(got, attr_nl_ref.decode(_plain(vals, bpv, ver, pts), *args)[0]), ver
        assert np.abs(got - vals).max() <= KINDS[ver][1], ver


def test_v8_known_answer_one_point():
    """Worked by hand.  One point, three uint8 channels (5, 5, 5), mask {1, 2}: n = 1 gives S = 1 and one chunk, the point
    is the first of lane 0's run, so version 1's residual is the value itself, w = (5, 5, 5), and the cross kind codes
    x = (5, 5 - 5, 5 - 5) = (5, 0, 0).  Head: 'A', version 8 (plain: 1), bpv 1, byte 3 = 3 | 3 << 4 = 0x33 (plain: 3).
    Decisions, all with bucket 0 (a run's first point), context = channel * 80 + position:
      channel 0, x = 5 = 0b101, k = 2: zero flag 1 (ctx 0), sign 0 (1), prefix 1, 1, 0 (2, 3, 4), suffix bit 1 of 5 = 0
        (ctx 2 + 7 + 1 = 10), bit 0 of 5 = 1 (ctx 9)
      channel 1, x = 0: zero flag 0 (ctx 80);  channel 2, x = 0: zero flag 0 (ctx 160)
    (the plain kind codes channel 0's seven decisions three times over, at ctx 80 .. and 160 ..: its p0 differ there.)
    p0 = (4096 (2 c1 + 1)) // (2 (c0 + c1 + 1)): a context that saw one one -> 3072 (ctx 0, 2, 3, 9), one zero -> 1024
    (ctx 1, 4, 10, 80, 160), unused -> 2048.
    rANS of lane 0, x0 = 65536, the decisions in reverse; a zero under p1 = 1024 and a one under p1 = 3072 both have
    freq 3072, the one has start 1024:
      ctx 160 bit 0: (65536 // 3072 << 12) + 65536 % 3072                 = 21 * 4096 + 1024        = 87040
      ctx 80  bit 0: 87040 = 28 * 3072 + 1024                            -> 28 * 4096 + 1024        = 115712
      ctx 9   bit 1: 115712 = 37 * 3072 + 2048                           -> 37 * 4096 + 2048 + 1024 = 154624
      ctx 10  bit 0: 154624 = 50 * 3072 + 1024                           -> 50 * 4096 + 1024        = 205824
      ctx 4   bit 0: 205824 = 67 * 3072 + 0                              -> 67 * 4096               = 274432
      ctx 3   bit 1: 274432 = 89 * 3072 + 1024                           -> 89 * 4096 + 1024 + 1024 = 366592
      ctx 2   bit 1: 366592 = 119 * 3072 + 1024                          -> 119 * 4096 + 2048       = 489472
      ctx 1   bit 0: 489472 = 159 * 3072 + 1024                          -> 159 * 4096 + 1024       = 652288
      ctx 0   bit 1: 652288 = 212 * 3072 + 1024                          -> 212 * 4096 + 2048       = 870400
    which never reaches freq << 20: no word is emitted, lane 0's state is 870400 = 0x000D4800, the other 63 lanes'
    0x00010000, every run of words is empty and the chunk is 128 state words + 64 lengths = 192 words."""
    vals = np.array([[5, 5, 5]])
    blob = attr_cross_ref.encode(vals, 1, True)
    p0 = [2048] * 240
    for k in (0, 2, 3, 9):
        p0[k] = 3072
    for k in (1, 4, 10, 80, 160):
        p0[k] = 1024
    body = struct.pack("<II", 1, 1) + struct.pack("<240H", *p0) + struct.pack("<I", 192)
    body += struct.pack("<128H", *([0x4800, 0x000D] + [0x0000, 0x0001] * 63)) + bytes(128)
    want = bytes([ord("A"), 8, 1, 0x33]) + struct.pack("<I", 1) + struct.pack("<I", len(body)) + body
    assert blob == want
    assert np.array_equal(attr_cross_ref.decode(blob)[0], vals)
    plain = attr_ref.encode(vals, 1)
    assert len(plain) == len(blob)
    differ = {i for i in range(len(blob)) if blob[i] != plain[i]}
    p0_at, states_at = 20, 20 + 480 + 4
    # against the plain blob: the two head bytes; the high bytes of p0 where channels 1 and 2 coded a 5 (3072 or 1024
    # at positions 0 .. 4, 9, 10) and now code a zero flag (1024 at position 0, 2048 elsewhere); lane 0's state
    state = set(range(states_at, states_at + 4))
    assert differ - state == {1, 3} | {p0_at + 2 * (ch + pos) + 1 for ch in (80, 160) for pos in (0, 1, 2, 3, 4, 9, 10)}
    assert differ & state
    assert GeometryCodec().attr_info(blob) == {"version": 8, "bpv": 1, "channels": 3, "points": 1, "max_error": 0, "scalable": False,
                                              "lod": 0, "cross_channel": (1, 2)}


def GeometryCodec():
    return pkg().GeometryCodec


def _zed(i):
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        u, mean = attr_ref.merge(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"])
    return _morton(u, mean)


@pytest.mark.parametrize("frame", [0, 20])
def test_recorded_colour_is_a_tenth_smaller_at_least(frame):
    """the size condition: on recorded camera frames the cross blob is at most 0.90 of the plain blob of the same kind
    (the coded bodies alone measure 0.77 - 0.81; heads, p0 and lane states are the same bytes in both)"""
    pts, vals = _zed(frame)
    for ver in sorted(KINDS):
        cross, plain = len(_encode(vals, 1, True, ver, pts)), len(_plain(vals, 1, ver, pts))
        print(f"frame {frame}, version {ver}: plain {plain} B, cross {cross} B ({cross / plain:.3f})")
        assert cross <= 0.90 * plain, (frame, ver, cross, plain)


def test_host_entry_points_against_the_restatement(clouds):
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    for name in ("pcc_attr_encode_frames_cross", "pcc_attr_cross_mask"):
        assert name + "(" in text and name in abi.PROTOTYPES and hasattr(abi.lib(), name)
    G = GeometryCodec()
    rng = np.random.default_rng(9)
    for n in (0, 1, 300):
        pts = clouds[n] if n else np.zeros((0, 3), np.int64)
        for c, cross in ((2, True), (3, (2,)), (4, (1, 2)), (4, True)):
            for bpv in (1, 2):
                vals = _correlated(rng, n, c, bpv) if n else np.zeros((0, c), np.int64)
                for ver in KINDS:
                    blob = _encode(vals, bpv, cross, ver, pts)
                    want = attr_cross_ref.info(blob)
                    assert want["version"] == ver and want["channels"] == c and want["points"] == n
                    assert want["cross_channel"] == ((1, 2, 3)[:c - 1] if cross is True else tuple(cross))
                    assert G.attr_info(blob) == want and G.attr_info(blob[:16]) == want, (n, c, cross, bpv, ver)
                    plain = _plain(vals, bpv, ver, pts)
                    assert "cross_channel" not in G.attr_info(plain) and G.attr_info(plain) == attr_nl_ref.info(plain)
                    if ver in (11, 14):
                        for k in (0, 1, 2, 5, 15):
                            w = attr_cross_ref.lod_info(blob, k)
                            assert G.attr_lod_info(blob, k) == w, (n, c, ver, k)
                            assert G.attr_lod_info(blob[:attr_cross_ref.lod_info(blob, max(k - 1, 0))[0]], k) == w, (n, c, ver, k)
                    else:
                        with pytest.raises(abi.PccError) as e:
                            G.attr_lod_info(blob, 1)
                        assert e.value.code == abi.PCC_E_ARG


def test_host_parse_refusals(clouds):
    """what the host parse refuses, each PCC_E_STREAM: the version bytes that are no kind, a cross byte with an empty
    mask or a bit at c - 1 and above, a plain byte with anything above the channels in byte 3"""
    abi = pkg("_abi")
    G = GeometryCodec()
    pts = clouds[300]
    vals = _correlated(np.random.default_rng(2), 300, 3, 1)

    def refused(bad, lod=None):
        with pytest.raises(abi.PccError) as e:
            G.attr_info(bad) if lod is None else G.attr_lod_info(bad, lod)
        assert e.value.code == abi.PCC_E_STREAM, (bad[:4], lod, str(e.value))
    for ver in (1, 2, 4, 7, 8, 11, 13, 14):
        cross = ver in KINDS
        blob = _encode(vals, 1, True, ver, pts) if cross else attr_nl_ref.encode(vals, 1, {4: 2, 7: 2}.get(ver, 0),
                                                                                 points=pts if ver in (2, 7) else None)
        assert G.attr_info(blob)["version"] == ver
        lod = 1 if ver in (2, 7, 11, 14) else None
        for other in (0, 3, 5, 6, 9, 10, 12, 15, 16, 0x81):
            refused(blob[:1] + bytes([other]) + blob[2:])
        if cross:
            for b3 in (3, 3 | (4 << 4), 3 | (8 << 4), 3 | (7 << 4), 2 | (2 << 4), 2 | (3 << 4), 1 | (1 << 4), 0 | (1 << 4), 5 | (1 << 4)):
                refused(blob[:3] + bytes([b3]) + blob[4:])                     # no mask; a bit at c - 1 or above; c itself
                if lod:
                    refused(blob[:3] + bytes([b3]) + blob[4:], lod)
            for b3 in (3 | (1 << 4), 3 | (2 << 4)):                            # another valid mask: still a well-formed head
                assert G.attr_info(blob[:3] + bytes([b3]) + blob[4:])["cross_channel"] == ((1,) if b3 >> 4 == 1 else (2,))
            empty = bytes([ord("A"), ver, 1, 0x33]) + bytes(8)
            assert G.attr_info(empty)["cross_channel"] == (1, 2) and G.attr_info(empty)["points"] == 0
            refused(bytes([ord("A"), ver, 1, 0x03]) + bytes(8))
            refused(bytes([ord("A"), ver, 1, 0x43]) + bytes(8))
        else:
            for b3 in (3 | (1 << 4), 3 | (3 << 4), 3 | (8 << 4)):
                refused(blob[:3] + bytes([b3]) + blob[4:])
                if lod:
                    refused(blob[:3] + bytes([b3]) + blob[4:], lod)
        refused(blob[:11])


def test_compress_checks_cross_channel():
    check = GeometryCodec()._check_cross
    a2, a4, a1 = np.zeros((3, 2), np.uint8), np.zeros((3, 4), np.uint16), np.zeros((3, 1), np.uint8)
    assert check(False, None) is None and check(False, [a2]) is None
    assert check(True, [a2, a4, a1]) == [1, 7, 0]
    assert check((1, 2), [a4]) == [3] and check([3, 1], [a4]) == [5] and check((1,), [a2, a4]) == [1, 1] and check((), [a1]) == [0]
    assert check((np.int64(2),), [a4]) == [2]
    for bad in (1, None, "12", 1.0, (1.0,), (True,), {1, 2}, np.array([1, 2])):
        with pytest.raises(TypeError):
            check(bad, [a4])
    for bad in ((0,), (4,), (1, 1), (-1,)):
        with pytest.raises(ValueError):
            check(bad, [a4])
    with pytest.raises(ValueError, match="frame 1:"):
        check((1, 2), [a4, a2])
    with pytest.raises(ValueError, match="frame 2:"):
        check((1,), [a4, a2, a1])
    with pytest.raises(ValueError, match="attributes"):
        check(True, None)
    with pytest.raises(ValueError, match="attributes"):
        check((1,), None)
