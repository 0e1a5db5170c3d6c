"""Transform-coded attribute blobs with a colour transform and one step per channel, version 21 (include/pcc.h has the
rule), on the host: the colour transform's known answers and its round trip, the numpy restatement
tests/attr_colour_ref.py against version 19's where the two must agree and through its own decoder, the condition on
recorded camera frames that the kind exists for, the host-only entry points with what they refuse, and what compress
refuses before it enters the runtime.  No GPU."""
import os
import struct

import numpy as np
import pytest

import attr2_ref
import attr_colour_ref as K
import attr_ref
import attr_transform_ref as T
from conftest import ROOT, pkg, random_cloud
from test_geometry_attributes_lod import _morton

GeometryCodec = pkg().GeometryCodec


def _cloud(rng, n, extent=60):
    pts = random_cloud(rng, n, extent=extent, lo=-30)[:, 1:]
    return pts[np.argsort(attr2_ref.keys_of(pts))]                          # Morton order: row i of the values is point i


def _smooth(rng, n, c, bpv):
    top = 1 << (8 * bpv)
    base = np.cumsum(rng.integers(-9, 10, n)) * (1 if bpv == 1 else 97) + rng.integers(0, top)
    return ((base[:, None] + rng.integers(-4, 5, (n, c)) * (1 if bpv == 1 else 50)) % top).astype(np.int64)


def test_the_colour_transform_known_answers_and_round_trip():
    """the four triples worked by hand (bpv = 1), and for both widths the eight corners of the colour cube and seeded
    random triples: every transformed value fits the value width, and the way back moves no channel by more than 1"""
    v = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]])
    fwd = K.colour_forward(v, 1)
    assert fwd.tolist() == [[255, 128, 128], [63, 255, 64], [127, 128, 255], [63, 0, 64]]
    back = K.colour_inverse(fwd[:2], 1)
    assert back.tolist() == [[255, 255, 255], [254, 0, 0]]                  # the second: G = -1 before the clamp
    rng = np.random.default_rng(21)
    for bpv in (1, 2):
        mask = (1 << (8 * bpv)) - 1
        corners = np.array([[(k >> 2 & 1) * mask, (k >> 1 & 1) * mask, (k & 1) * mask, 77] for k in range(8)])
        for v in (corners, rng.integers(0, mask + 1, (20000, 3))):
            f = K.colour_forward(v, bpv)
            assert f.min() >= 0 and f.max() <= mask
            b = K.colour_inverse(f, bpv)
            assert np.abs(b - v).max() <= 1
            assert v.shape[1] == 3 or (np.array_equal(f[:, 3], v[:, 3]) and np.array_equal(b[:, 3], v[:, 3]))      # a fourth channel is untouched
        f = K.colour_forward(corners, bpv)
        assert f[:, 1].min() == 0 and f[:, 1].max() == mask and f[:, 2].max() == mask      # Co reaches both ends, Cg the upper


def test_equal_steps_without_colour_are_version_19():
    """with all q[ch] equal and colour 0 the indices are version 19's and so are the bytes behind the heads"""
    rng = np.random.default_rng(5)
    for n, c, bpv, q in ((300, 3, 1, 7), (65, 2, 2, 700), (2, 4, 1, 1)):
        pts, vals = _cloud(rng, n), _smooth(rng, n, c, bpv)
        b19, b21 = T.encode(pts, vals, bpv, q), K.encode(pts, vals, bpv, q)
        assert b21 == K.encode(pts, vals, bpv, (q,) * c, 0)
        assert np.array_equal(K.indices(b21), T.indices(b19))
        assert b21[:4] == bytes([ord("A"), 21, bpv, c]) and b21[4:8] == b19[4:8]
        assert struct.unpack_from("<I", b21, 8)[0] == struct.unpack_from("<I", b19, 8)[0] + 4 * c
        assert b21[12:16 + 4 * c] == struct.pack("<%dI" % (1 + c), 0, *[q] * c)
        assert b21[16 + 4 * c:] == b19[16:]
        assert np.array_equal(K.reconstruct(pts, vals, bpv, q), T.reconstruct(pts, vals, bpv, q))
    # steps that differ change the channel they belong to, and that channel only
    pts, vals = _cloud(rng, 300), _smooth(rng, 300, 3, 1)
    keys = np.sort(attr2_ref.keys_of(pts))
    x = K.forward(keys, vals, (3, 9, 17), 1)
    for ch, q in enumerate((3, 9, 17)):
        assert np.array_equal(x[:, ch], T.forward(keys, vals[:, ch:ch + 1], q, 1)[:, 0])


def test_round_trip_of_the_restatement():
    """decode(encode(..)) is reconstruct(..) at 1, 2, 65 and 300 points, with and without the transform, both widths"""
    rng = np.random.default_rng(6)
    for n in (1, 2, 65, 300):
        pts = _cloud(rng, n)
        for bpv, c, q, colour in ((1, 3, 16, 1), (1, 4, (5, 11, 11, 2), 1), (2, 3, (300, 900, 900), 1), (1, 3, (3, 9, 17), 0),
                                  (2, 2, (70, 7000), 0)):
            vals = _smooth(rng, n, c, bpv)
            blob = K.encode(pts, vals, bpv, q, colour)
            got, gb = K.decode(blob, pts)
            assert gb == bpv and np.array_equal(got, K.reconstruct(pts, vals, bpv, q, colour)), (n, bpv, c, q, colour)
            i = K.info(blob)
            assert i["colour"] == ("ycocg" if colour else None) and i["qstep"] == ((q,) * c if isinstance(q, int) else q)
    # one point: the mean alone is exact, so the colour round trip is all that moves it
    got = K.decode(K.encode(np.array([[1, 2, 3]]), np.array([[255, 0, 0]]), 1, 9, 1), np.array([[1, 2, 3]]))[0]
    assert got.tolist() == [[254, 0, 0]]
    # the sender's side of a level of detail, and no points
    cells = np.unique(_cloud(rng, 300) >> 2, axis=0)
    vals = _smooth(rng, cells.shape[0], 3, 1)
    blob = K.encode(cells, vals, 1, 12, 1, 32768 >> 2)
    assert blob[2] == 1 | (2 << 4) and np.array_equal(K.decode(blob, cells)[0], K.reconstruct(cells, vals, 1, 12, 1, 32768 >> 2))
    assert K.encode(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), 1, 5, 1) == bytes([ord("A"), 21, 1, 3]) + bytes(8)


def _zed(i):
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        u, mean = attr_ref.merge(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"])
    return _morton(u, mean)


def test_recorded_colour_is_smaller_and_closer_than_plain_rgb():
    """what the kind is for: on every one of the 25 recorded frames the colour blob at q = 16 is shorter than version
    19's at q = 32 and its mean squared error over R, G, B is lower (measured where the kind was proposed: bytes 0.864 -
    0.928 of the plain blob's, MSE 0.64 - 0.80 of it)"""
    for i in range(25):
        pts, vals = _zed(i)
        vals = np.asarray(vals, np.int64)
        c_blob = K.encode(pts, vals, 1, 16, 1)
        c_mse = float(((K.reconstruct(pts, vals, 1, 16, 1) - vals) ** 2).mean())
        t_blob = T.encode(pts, vals, 1, 32)
        t_mse = float(((T.reconstruct(pts, vals, 1, 32) - vals) ** 2).mean())
        print(f"frame {i} ({len(pts)} points): ycocg q=16 {len(c_blob)} B, mse {c_mse:.1f}; plain q=32 {len(t_blob)} B, mse {t_mse:.1f}")
        assert len(c_blob) < len(t_blob) and c_mse < t_mse, (i, len(c_blob), len(t_blob), c_mse, t_mse)


def test_host_parse_and_refusals():
    """pcc_attr_info and pcc_attr_transform_info on version 21: what they read back, from the blob and from a prefix of
    16 + 4 c bytes, and what they refuse, each PCC_E_STREAM"""
    abi = pkg("_abi")
    rng = np.random.default_rng(3)
    pts = _cloud(rng, 300)
    vals = _smooth(rng, 300, 3, 1)
    blob = K.encode(pts, vals, 1, (5, 11, 12), 1)
    want = {"version": 21, "bpv": 1, "channels": 3, "points": 300, "qstep": (5, 11, 12), "colour": "ycocg", "max_error": 0,
            "scalable": False, "lod": 0}
    assert GeometryCodec.attr_info(blob) == want == K.info(blob)
    head = 16 + 4 * 3 + 8
    for cut in (28, 29, head - 1, head, 100, head + 2 * 240 + 2, len(blob) - 1):
        assert GeometryCodec.attr_info(blob[:cut]) == want, cut
    plain = K.encode(pts, vals, 1, 9)
    assert GeometryCodec.attr_info(plain) == dict(want, qstep=(9, 9, 9), colour=None) == K.info(plain)
    cells = np.unique(pts >> 3, axis=0)
    b16 = K.encode(cells, _smooth(rng, cells.shape[0], 4, 2), 2, (32767, 1, 2, 3), 1, 32768 >> 3)
    i16 = GeometryCodec.attr_info(b16)
    assert i16 == K.info(b16) and (i16["bpv"], i16["channels"], i16["qstep"], i16["colour"], i16["lod"]) == (2, 4, (32767, 1, 2, 3), "ycocg", 3)
    empty = bytes([ord("A"), 21, 1 | (15 << 4), 4]) + bytes(8)
    assert GeometryCodec.attr_info(empty) == {"version": 21, "bpv": 1, "channels": 4, "points": 0, "qstep": (0, 0, 0, 0), "colour": None,
                                              "max_error": 0, "scalable": False, "lod": 15} == K.info(empty)
    # version 19's dict is unchanged, and pcc_attr_qstep says 0 for version 21
    b19 = T.encode(pts, vals, 1, 32)
    assert GeometryCodec.attr_info(b19) == T.info(b19) and "colour" not in GeometryCodec.attr_info(b19)
    import ctypes as C
    buf = np.frombuffer(blob, np.uint8)
    q = C.c_int32(-1)
    assert abi.lib().pcc_attr_qstep(C.c_void_p(buf.ctypes.data), len(blob), C.byref(q)) == 0 and q.value == 0
    col, steps = C.c_int32(-1), (C.c_int32 * 4)(-1, -1, -1, -1)
    b19buf = np.frombuffer(b19, np.uint8)
    assert abi.lib().pcc_attr_transform_info(C.c_void_p(b19buf.ctypes.data), len(b19), C.byref(col), steps) == 0
    assert col.value == 0 and list(steps) == [0, 0, 0, 0]

    def refused(bad, code=abi.PCC_E_STREAM, lod=None):
        with pytest.raises(abi.PccError) as e:
            GeometryCodec.attr_info(bad) if lod is None else GeometryCodec.attr_lod_info(bad, lod)
        assert e.value.code == code, (bad[:16], str(e.value))

    def patched(at, fmt, *v, of=blob):
        return of[:at] + struct.pack(fmt, *v) + of[at + struct.calcsize(fmt):]
    refused(patched(12, "<I", 2))                                           # a colour word above 1
    refused(patched(12, "<I", 2)[:28])
    two = K.encode(pts, vals[:, :2], 1, 9)
    assert GeometryCodec.attr_info(two)["colour"] is None
    refused(patched(12, "<I", 1, of=two))                                   # the transform with 2 channels
    for ch in range(3):
        refused(patched(16 + 4 * ch, "<I", 0))                              # a step of 0, of H
        refused(patched(16 + 4 * ch, "<I", 128))
        refused(patched(16 + 4 * ch, "<I", 128)[:28])
    refused(patched(16, "<I", 32768, of=b16))
    refused(blob[:27])                                                      # q[c - 1] is cut
    table = head + 2 * 240
    cut = blob[:table + 2]                                                  # a blob that ends inside its chunk table
    refused(cut[:8] + struct.pack("<I", len(cut) - 12) + cut[12:])
    words = struct.unpack_from("<I", blob, table)[0]
    refused(patched(table, "<I", words + 1))                                # words that do not add up
    refused(patched(8, "<I", len(blob) - 12 + 2))                           # a payload_len the chunks do not fill
    for b3 in (0, 5, 3 | (1 << 4)):
        refused(patched(3, "B", b3))
    for b2 in (0, 3, 3 | (2 << 4)):
        refused(patched(2, "B", b2))
    refused(patched(head - 8, "<I", 3))                                     # S that does not hold the points
    refused(patched(head - 4, "<I", 2))                                     # one chunk too many for them
    refused(patched(head, "<H", 5000))                                      # an initial probability out of range
    refused(bytes([ord("A"), 21, 1, 3]) + struct.pack("<II", 0, 4) + bytes(4))      # no points, a payload
    for other in (20, 22, 23, 29, 5, 53, 0x95):                             # neighbours of 21 are no kind
        refused(patched(1, "B", other))
    refused(blob, abi.PCC_E_ARG, lod=0)                                     # no levels of detail, as version 19
    refused(blob, abi.PCC_E_ARG, lod=1)


def test_byte_21_against_the_rule_of_the_version_bytes():
    """odd parity, so two bits from each of the other nine"""
    kinds = (1, 2, 4, 7, 8, 11, 13, 14, 19)
    assert bin(21).count("1") % 2 == 1 and all(bin(k).count("1") % 2 == 1 for k in kinds)
    assert all(bin(21 ^ k).count("1") >= 2 for k in kinds)


def test_abi_is_declared_and_bound():
    abi = pkg("_abi")
    with open(os.path.join(ROOT, "include", "pcc.h")) as f:
        text = f.read()
    for name in ("pcc_attr_encode_frames_transform2", "pcc_attr_transform_info"):
        assert name in abi.PROTOTYPES and name + "(" in text, name
        assert getattr(abi.lib(), name) is not None


def test_compress_checks_colour_and_the_steps():
    """the checks of compress that run before the runtime is entered: on an instance that has none"""
    geo = object.__new__(GeometryCodec)
    pts = [np.zeros((3, 3), np.int32) + np.arange(3, dtype=np.int32)[:, None]] * 2
    a8, a16, a84, a82 = np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.uint16), np.zeros((3, 4), np.uint8), np.zeros((3, 2), np.uint8)
    for bad in ((4, True, 4), (4, 1.0, 4), [4, "4", 4], (4, None, 4), (np.float32(2), 4, 4)):
        with pytest.raises(TypeError, match="qstep"):
            geo.compress(pts, attributes=[a8, a8], qstep=bad)
        with pytest.raises(TypeError, match="qstep"):
            geo.compress(pts, attributes=[a8, a8], qstep=bad, colour="ycocg")
    with pytest.raises(ValueError, match="frame 0: qstep 0 of channel 1"):
        geo.compress(pts, attributes=[a8, a8], qstep=(4, 0, 4))
    with pytest.raises(ValueError, match="frame 1: qstep 128 of channel 2"):
        geo.compress(pts, attributes=[a16, a8], qstep=[4, 4, 128])
    with pytest.raises(ValueError, match="frame 0: qstep 32768 of channel 0"):
        geo.compress(pts, attributes=[a16, a16], qstep=(32768, 1, 1), colour="ycocg")
    with pytest.raises(ValueError, match="frame 1: qstep 128"):
        geo.compress(pts, attributes=[a16, a8], qstep=128, colour="ycocg")
    with pytest.raises(ValueError, match="frame 1: qstep has 3 steps, the frame has 4 channels"):
        geo.compress(pts, attributes=[a8, a84], qstep=(4, 4, 4))
    with pytest.raises(ValueError, match="frame 0: qstep has 4 steps, the frame has 3 channels"):
        geo.compress(pts, attributes=[a8, a84], qstep=(4, 4, 4, 4), colour="ycocg")
    with pytest.raises(ValueError, match="frame 0: qstep has 0 steps"):
        geo.compress(pts, attributes=[a8, a8], qstep=())
    with pytest.raises(ValueError, match="attributes="):
        geo.compress(pts, qstep=(4, 4, 4))
    with pytest.raises(ValueError, match="cross_channel="):                 # colour without qstep: where to look instead
        geo.compress(pts, attributes=[a8, a8], colour="ycocg")
    with pytest.raises(ValueError, match="cross_channel="):
        geo.compress(pts, attributes=[a8, a8], qstep=0, colour="ycocg")
    with pytest.raises(ValueError, match="frame 1: colour='ycocg' needs 3 channels"):
        geo.compress(pts, attributes=[a8, a82], qstep=4, colour="ycocg")
    for bad in ("rgb", "YCoCg", 1, True, b"ycocg"):
        with pytest.raises(ValueError, match="colour must be"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, colour=bad)
    for kw in (dict(qstep=(4, 4, 4)), dict(qstep=4, colour="ycocg"), dict(qstep=(4, 8, 8), colour="ycocg")):
        with pytest.raises(ValueError, match="max_error: a transform-coded blob"):
            geo.compress(pts, attributes=[a8, a8], max_error=1, **kw)
        with pytest.raises(ValueError, match="scalable=True: a transform-coded blob"):
            geo.compress(pts, attributes=[a8, a8], scalable=True, **kw)
        with pytest.raises(ValueError, match="has no cross-channel form"):
            geo.compress(pts, attributes=[a8, a8], cross_channel=True, **kw)
    check = geo._check_colour
    assert check(0, None, None, 0, False, None) == (0, None, 0) and check(7, None, [a8], 0, False, None) == (7, None, 0)
    assert check(7, "ycocg", [a8, a84], 0, False, None) == (1, [7, 7, 7, 7], 1)
    assert check((127, 1, 2), None, [a8], 0, False, None) == (1, [127, 1, 2], 0)
    assert check([32767, 1, np.int64(2)], "ycocg", [a16], 0, False, None) == (1, [32767, 1, 2], 1)
