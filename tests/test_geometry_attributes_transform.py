"""Transform-coded attribute blobs, version 19 (include/pcc.h has the rule), on the host: the numpy restatement
tests/attr_transform_ref.py on one blob worked by hand and on the shapes where the rule or the layout changes, the
condition on recorded camera frames that the kind exists for, the host-only entry points (pcc_attr_info,
pcc_attr_qstep, pcc_attr_lod_info) with what they refuse, and what compress refuses before it enters the runtime.
No GPU."""
import os
import struct

import numpy as np
import pytest

import attr2_ref
import attr_nl_ref
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


def test_a_blob_worked_by_hand():
    """Three points, one uint8 channel, q = 4; H = 128, mask = 255.  With bias 32768 every coordinate has bit 15 set, so
    K = 7 << 45 is the key of (0, 0, 0); x sits at bit 3 i + 2, y at 3 i + 1, z at 3 i of a key:

        point      key     v     b
        (0, 0, 0)  K       60    48   (the first point)
        (0, 0, 1)  K | 1   11    0    hb((K | 1) ^ K)
        (1, 0, 0)  K | 4   200   2    hb((K | 4) ^ (K | 1)) = hb(5)

    Forward, sublevel 0, i = 1: lo = lower_bound(K) = 0, hi = lower_bound(K + 2) = 2, wa = wb = 1, w = 2;
      h = 11 - 60 = -49; val[0] = 60 + floor(-49 / 2) = 60 - 25 = 35; s = max(2, isqrt(16 * 2 / 1)) = isqrt(32) = 5;
      x[1] = -floor((49 + 2) / 5) = -10.
    Sublevel 2, i = 2: lo = lower_bound(K) = 0, hi = lower_bound((K | 7) + 1) = 3, wa = 2, wb = 1, w = 3;
      h = 200 - 35 = 165; val[0] = 35 + floor(165 / 3) = 90; s = max(2, isqrt(floor(16 * 3 / 2))) = isqrt(24) = 4;
      x[2] = floor((165 + 2) / 4) = 41.
    x[0] = 90 - 128 = -38.  Coding order (b descending): points 0, 2, 1 -> -38, 41, -10.
    Inverse: val[0] = 90.  Sublevel 2: h^ = 41 * 4 = 164, va = 90 - floor(164 / 3) = 36, val[2] = 200.
      Sublevel 0: h^ = -10 * 5 = -50, va = 36 - floor(-50 / 2) = 36 + 25 = 61, val[1] = 61 - 50 = 11.  Values 61, 11, 200.
    Layout: attr_layout(3, 1) gives S = 1 and one chunk, so the three indices open the runs of lanes 0, 1, 2."""
    pts = np.array([[0, 0, 1], [1, 0, 0], [0, 0, 0]])
    vals = np.array([11, 200, 60])
    K = 7 << 45
    keys = np.sort(attr2_ref.keys_of(pts))
    assert keys.tolist() == [K, K | 1, K | 4]
    b = T.sublevels(keys)
    assert b.tolist() == [48, 0, 2] and T.order_of(b).tolist() == [0, 2, 1]
    assert [a.tolist() for a in T.pairs(keys, b, 0)] == [[1], [0], [1], [1]]
    assert [a.tolist() for a in T.pairs(keys, b, 2)] == [[2], [0], [2], [1]]
    assert T.step(4, 1, 1) == 5 and T.step(4, 2, 1) == 4
    x = T.forward(keys, np.array([[60], [11], [200]]), 4, 1)
    assert x[:, 0].tolist() == [-38, -10, 41]
    assert T.inverse(keys, x, 4, 1)[:, 0].tolist() == [61, 11, 200]
    blob = T.encode(pts, vals, 1, 4)
    head = bytes([ord("A"), 19, 1, 1]) + struct.pack("<II", 3, len(blob) - 12) + struct.pack("<III", 4, 1, 1)
    assert blob[:24] == head
    nctx = 1 * 5 * 16
    assert struct.unpack_from("<I", blob, 24 + 2 * nctx)[0] * 2 == len(blob) - (24 + 2 * nctx + 4)      # the one chunk's words
    assert T.indices(blob)[:, 0].tolist() == [-38, 41, -10]
    got, bpv = T.decode(blob, pts)
    assert bpv == 1 and got[:, 0].tolist() == [61, 11, 200]
    assert T.info(blob) == {"version": 19, "bpv": 1, "channels": 1, "points": 3, "qstep": 4, "max_error": 0, "scalable": False,
                            "lod": 0}


def _round_trip(pts, vals, bpv, q, bias=32768):
    blob = T.encode(pts, vals, bpv, q, bias)
    want = T.reconstruct(pts, vals, bpv, q, bias)
    got, gb = T.decode(blob, pts)
    assert gb == bpv and np.array_equal(got, want), (len(pts), bpv, q)
    return blob, got


def test_round_trip_of_the_restatement():
    rng = np.random.default_rng(19)
    H8 = 128
    # n = 1: the mean alone, exact
    blob, got = _round_trip(np.array([[3, -4, 5]]), np.array([[200, 0, 77]]), 1, 9)
    assert got.tolist() == [[200, 0, 77]] and T.indices(blob).tolist() == [[200 - H8, -H8, 77 - H8]]
    # n = 2, split at bit 0 (z differs in its lowest bit) and at bit 47 (x differs in its highest, across the bias)
    for pts, bit in ((np.array([[2, 2, 2], [2, 2, 3]]), 0), (np.array([[-1, 5, 5], [0, 5, 5]]), 47)):
        assert T.sublevels(np.sort(attr2_ref.keys_of(pts))).tolist() == [48, bit]
        for q in (1, 7, 127):
            _round_trip(pts, np.array([[10, 250], [245, 3]]), 1, q)
    # |h| = mask under s = 2 reaches the clamp of the index
    pts = _cloud(rng, 64)
    vals = (np.arange(64) % 2 * 255)[:, None].astype(np.int64)
    keys = np.sort(attr2_ref.keys_of(pts))
    x = T.forward(keys, vals, 1, 1)
    assert (np.abs(x[1:]) == H8 - 1).any() and np.abs(x[1:]).max() == H8 - 1
    _round_trip(pts, vals, 1, 1)
    v16 = (np.arange(64) % 2 * 65535)[:, None].astype(np.int64)
    assert np.abs(T.forward(keys, v16, 1, 2)[1:]).max() == 32767
    _round_trip(pts, v16, 2, 1)
    # uint16 x 2, uint8 x 4; n at both sides of a lane-run boundary (S = 1 | 2) and of a chunk boundary (attr_layout)
    assert attr_ref.layout(64, 2) == (1, 1) and attr_ref.layout(65, 2) == (2, 1)
    assert attr_ref.layout(8192, 4) == (128, 1) and attr_ref.layout(8193, 4)[1] == 2
    for n in (64, 65, 300):
        pts = _cloud(rng, n)
        _round_trip(pts, _smooth(rng, n, 2, 2), 2, 700)
        _round_trip(pts, _smooth(rng, n, 4, 1), 1, 5)
    for n in (8192, 8193):
        pts = _cloud(rng, n, extent=96)
        blob, _ = _round_trip(pts, _smooth(rng, n, 4, 1), 1, 16)
        assert struct.unpack_from("<II", blob, 16) == attr_ref.layout(n, 4)
    # the sender's side of a level of detail: cells under bias 32768 >> 2
    cells = np.unique(_cloud(rng, 300) >> 2, axis=0)
    blob, _ = _round_trip(cells, _smooth(rng, cells.shape[0], 3, 1), 1, 12, 32768 >> 2)
    assert blob[2] == 1 | (2 << 4)
    # no points
    assert T.encode(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), 1, 5) == bytes([ord("A"), 19, 1, 3]) + bytes(8)


def _zed(i):
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        u, mean = attr_ref.merge(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"])
    return _morton(u, mean)


def test_recorded_colour_is_smaller_and_closer_than_the_bounded_kind():
    """what the kind is for: on every one of the 25 recorded frames the q = 32 blob is shorter than version 4's at
    max_error = 16 and its mean squared error is lower (measured: 5 - 7 % fewer bytes, MSE 43 - 49 against 71 - 75)"""
    for i in range(25):
        pts, vals = _zed(i)
        vals = np.asarray(vals, np.int64)
        t_blob = T.encode(pts, vals, 1, 32)
        t_mse = float(((T.reconstruct(pts, vals, 1, 32) - vals) ** 2).mean())
        nl_blob = attr_nl_ref.encode(vals, 1, 16)
        nl_mse = float(((attr_nl_ref.decode(nl_blob)[0] - vals) ** 2).mean())
        print(f"frame {i} ({len(pts)} points): transform {len(t_blob)} B, mse {t_mse:.1f}; version 4 {len(nl_blob)} B, mse {nl_mse:.1f}")
        assert len(t_blob) < len(nl_blob) and t_mse < nl_mse, (i, len(t_blob), len(nl_blob), t_mse, nl_mse)


def test_host_parse_and_refusals():
    """pcc_attr_info on version 19: what it reads back, from the blob and from a prefix of 16 bytes, and what it refuses,
    each PCC_E_STREAM.  (A sender's level of detail above 15 cannot be written: byte 2 gives it one nibble; the other
    nibble, the bytes per value, is held to 1 and 2.)"""
    abi = pkg("_abi")
    rng = np.random.default_rng(3)
    pts = _cloud(rng, 300)
    blob = T.encode(pts, _smooth(rng, 300, 3, 1), 1, 32)
    want = {"version": 19, "bpv": 1, "channels": 3, "points": 300, "qstep": 32, "max_error": 0, "scalable": False, "lod": 0}
    assert GeometryCodec.attr_info(blob) == want == T.info(blob)
    assert GeometryCodec.attr_info(blob[:16]) == want
    for cut in (17, 23, 24, 100, 24 + 2 * 240 + 2, len(blob) - 1):
        assert GeometryCodec.attr_info(blob[:cut]) == want, cut
    cells = np.unique(pts >> 3, axis=0)
    b16 = T.encode(cells, _smooth(rng, cells.shape[0], 2, 2), 2, 32767, 32768 >> 3)
    i16 = GeometryCodec.attr_info(b16)
    assert (i16["version"], i16["bpv"], i16["channels"], i16["qstep"], i16["lod"]) == (19, 2, 2, 32767, 3)
    empty = bytes([ord("A"), 19, 1 | (15 << 4), 4]) + bytes(8)
    assert GeometryCodec.attr_info(empty) == {"version": 19, "bpv": 1, "channels": 4, "points": 0, "qstep": 0, "max_error": 0,
                                              "scalable": False, "lod": 15}

    def refused(bad, code=abi.PCC_E_STREAM, lod=None):
        with pytest.raises(abi.PccError) as e:
            GeometryCodec.attr_info(bad) if lod is None else GeometryCodec.attr_lod_info(bad, lod)
        assert e.value.code == code, (bad[:16], str(e.value))

    def patched(at, fmt, *v):
        return blob[:at] + struct.pack(fmt, *v) + blob[at + struct.calcsize(fmt):]
    refused(patched(12, "<I", 0))                                           # q = 0
    refused(patched(12, "<I", 128))                                         # q = H
    refused(patched(12, "<I", 0)[:16])
    refused(patched(12, "<I", 128)[:16])
    refused(b16[:12] + struct.pack("<I", 32768) + b16[16:])
    refused(blob[:15])                                                      # q is cut
    table = 24 + 2 * 240
    cut = blob[:table + 2]                                                  # a blob that ends inside its chunk table
    refused(cut[:8] + struct.pack("<I", len(cut) - 12) + cut[12:])
    words = struct.unpack_from("<I", blob, table)[0]
    refused(patched(table, "<I", words + 1))                                # words that do not add up
    refused(patched(table, "<I", words - 1))
    refused(patched(8, "<I", len(blob) - 12 + 2))                           # a payload_len the chunks do not fill
    for b3 in (0, 5, 3 | (1 << 4), 0x83):                                   # byte 3 outside 1 .. 4
        refused(patched(3, "B", b3))
    for b2 in (0, 3, 4, 3 | (2 << 4)):                                      # bytes per value outside 1, 2
        refused(patched(2, "B", b2))
    refused(patched(16, "<I", 3))                                           # S that does not hold the points
    refused(patched(20, "<I", 2))                                           # one chunk too many for them
    refused(patched(24, "<H", 5000))                                        # an initial probability out of range
    refused(bytes([ord("A"), 19, 1, 3]) + struct.pack("<II", 0, 4) + bytes(4))      # no points, a payload
    for other in (0, 3, 5, 6, 9, 10, 12, 15, 16, 17, 18, 23, 27, 51, 0x93):         # neighbours of 19 are no kind
        refused(patched(1, "B", other))
    # levels of detail are not a property of this kind: the convention of the run kinds
    refused(blob, abi.PCC_E_ARG, lod=0)
    refused(blob, abi.PCC_E_ARG, lod=1)


def test_abi_is_declared_and_bound():
    abi = pkg("_abi")
    with open(os.path.join(ROOT, "include", "pcc.h")) as f:
        text = f.read()
    for name in ("pcc_attr_encode_frames_transform", "pcc_attr_qstep"):
        assert name in abi.PROTOTYPES and name + "(" in text, name
        assert getattr(abi.lib(), name) is not None


def test_compress_checks_qstep():
    """the checks of compress that run before the runtime is entered: on an instance that has none"""
    geo = object.__new__(GeometryCodec)
    pts = [np.zeros((3, 3), np.int32) + np.arange(3, dtype=np.int32)[:, None]] * 2
    a8, a16 = np.zeros((3, 3), np.uint8), np.zeros((3, 2), np.uint16)
    for bad in (True, False, 1.0, "4", None, (4,), np.float32(2)):
        with pytest.raises(TypeError, match="qstep"):
            geo.compress(pts, attributes=[a8, a8], qstep=bad)
    with pytest.raises(ValueError, match="qstep"):
        geo.compress(pts, attributes=[a8, a8], qstep=-1)
    with pytest.raises(ValueError, match="attributes="):
        geo.compress(pts, qstep=4)
    with pytest.raises(ValueError, match="frame 1: qstep 128"):
        geo.compress(pts, attributes=[a16, a8], qstep=128)
    with pytest.raises(ValueError, match="frame 0: qstep 32768"):
        geo.compress(pts, attributes=[a16, a16], qstep=32768)
    with pytest.raises(ValueError, match="max_error"):
        geo.compress(pts, attributes=[a8, a8], qstep=4, max_error=1)
    with pytest.raises(ValueError, match="scalable"):
        geo.compress(pts, attributes=[a8, a8], qstep=4, scalable=True)
    with pytest.raises(ValueError, match="cross_channel"):
        geo.compress(pts, attributes=[a8, a8], qstep=4, cross_channel=True)
    with pytest.raises(ValueError, match="cross_channel"):
        geo.compress(pts, attributes=[a8, a8], qstep=np.int64(4), cross_channel=(1,))
    check = geo._check_qstep
    assert check(0, None, 0, False, None) == 0 and check(0, [a8], 3, True, [3]) == 0
    assert check(127, [a8], 0, False, None) == 127 and check(np.int32(32767), [a16], 0, False, None) == 32767
