"""Near-lossless attributes with a bounded error: attribute blob versions 4 and 7 (include/pcc.h has the rule,
csrc/attr_blob.h the layout; pcc_attr_encode_frames_nl / pcc_attr_info, GeometryCodec.compress(max_error=e) / attr_info).
Every near-lossless blob must equal the numpy restatement's (tests/attr_nl_ref.py) bytes, every decoded value the
restatement's, and no decoded value may be off by more than e from what the lossless coder returns for the same call."""
import os
import struct

import numpy as np
import pytest

import attr2_ref
import attr_nl_ref
import attr_ref
from conftest import ROOT, pkg, random_cloud
from test_geometry_attributes import _expected, _mixed
from test_geometry_attributes_lod import _morton, _sample, _values
from test_geometry_frames import _unique
from test_geometry_lod import _grid_cloud

ES = (1, 2, 7)


def _recon(pts, vals, e, scalable):
    """points / merged values in Morton order -> what a decoder returns at lod 0: the loop's reconstructions, clamped"""
    vals = np.asarray(vals, np.int64)
    if vals.shape[0] == 0 or e == 0:
        return vals
    if scalable:
        s, _, first = attr2_ref.intro(attr2_ref.keys_of(pts))
        vh = attr_nl_ref.indices7(vals, s, first, e)[1]
    else:
        vh = attr_nl_ref.indices4(vals, e)[1]
    return vh


def _clip(vh, bpv):
    return np.clip(vh, 0, (1 << (8 * bpv)) - 1)


def test_nl_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    for name in ("pcc_attr_encode_frames_nl", "pcc_attr_info"):
        assert name + "(" in text
        assert name in abi.PROTOTYPES
        assert hasattr(abi.lib(), name)
    assert abi.lib().pcc_abi_version() == 1
    for word in ("sgn(d) floor((|d| + e) / q)", "clamp(v^, 0, mask)", "q = 2 e + 1"):      # the rule, in full
        assert word in text, word


def test_restatement_hand_worked_streams():
    """(a) Version 4, one point, one uint8 channel, value 5, e = 1: q = 3, p = 0, d = 5, j = floor((5 + 1) / 3) = 2,
    v^ = 6 (|5 - 6| <= 1).  j = 2 = 0b10, k = 1.  Decisions (context: position of channel 0, bucket 0): zero flag 1 (0),
    sign 0 (1), prefix 1, 0 (2, 3), suffix bit 0 = 0 (2 + 7 + 0 = 9).  p0: a context that saw one one -> 3072, one zero ->
    1024, nothing -> 2048.  rANS from x = 65536, decisions in reverse (freq 3072 each; start 1024 for a one):
      ctx 9 bit 0:  21 * 4096 + 1024 = 87040             ctx 3 bit 0:  28 * 4096 + 1024 = 115712
      ctx 2 bit 1:  37 * 4096 + 2048 + 1024 = 154624     ctx 1 bit 0:  50 * 4096 + 1024 = 205824
      ctx 0 bit 1:  67 * 4096 + 0 + 1024 = 275456 = 0x00043400; no word
    The blob: version byte 4, payload_len counts max_error = 1, which stands directly behind it, then S = 1, one chunk of
    192 words as version 1 has them.
    (b) Version 7 of the same point: the same stream under version 2's head — max_error, then cells[16] = 1.
    (c) Version 7, three points (0,0,0), (0,0,1), (0,0,2), values 10, 12, 9, e = 1 (the points and their introduction
    order 0, 2, 1 with first = 0 for both are worked in test_geometry_attributes_lod): point 0: d = 10, j = floor(11 / 3) =
    3, v^ = 9; point 2: d = 9 - 9 = 0, j = 0, v^ = 9; point 1: d = 12 - 9 = 3, j = floor(4 / 3) = 1, v^ = 12.  Indices in
    introduction order 3, 0, 1; decoded 9, 12, 9; at lod 1 the cells' first points 0 and 2: 9 and 9.
    (d) Version 4, a run of three points (130 points give S = 3), uint8 values 10, 250, 0 with e = 2, q = 5: s = 0:
    p = 0, d = 10, j = 2, v^ = 10; s = 1: p = 10, d = 240, j = floor(242 / 5) = 48, v^ = 250; s = 2: p = (250 + 10 + 1)
    >> 1 = 130, d = -130, j = -floor(132 / 5) = -26, v^ = 0.  With 10, 254, 0 at e = 7, q = 15: j = 1, v^ = 15; p = 15,
    d = 239, j = floor(246 / 15) = 16, v^ = 255; p = (255 + 15 + 1) >> 1 = 135, d = -135, j = -floor(142 / 15) = -9,
    v^ = 0.  And 3, 255 at e = 7: j = 0, v^ = 0; d = 255, j = 17, v^ = 255; at e = 127, q = 255: 200 -> j = 1, v^ = 255
    (unclamped, inside 200 +- 127), then 0: p = 255, d = -255, j = -floor(382 / 255) = -1, v^ = 0."""
    p0 = [2048] * 80
    for k in (0, 2):
        p0[k] = 3072
    for k in (1, 3, 9):
        p0[k] = 1024
    tail = struct.pack("<II", 1, 1) + struct.pack("<80H", *p0) + struct.pack("<I", 192)
    tail += struct.pack("<128H", *([0x3400, 0x0004] + [0x0000, 0x0001] * 63)) + struct.pack("<64H", *([0] * 64))
    body = struct.pack("<I", 1) + tail
    want4 = bytes([ord("A"), 4, 1, 1]) + struct.pack("<II", 1, len(body)) + body
    assert attr_nl_ref.encode(np.array([5], np.uint8), 1, 1) == want4
    v, bpv = attr_nl_ref.decode(want4)
    assert bpv == 1 and v.tolist() == [[6]]
    assert attr_nl_ref.encode(np.zeros((0, 3), np.uint8), 1, 1) == bytes([ord("A"), 4, 1, 3]) + bytes(8)
    one = np.array([[3, -4, 5]])
    body = struct.pack("<I", 1) + struct.pack("<16I", *([1] * 16)) + tail
    want7 = bytes([ord("A"), 7, 1, 1]) + struct.pack("<II", 1, len(body)) + body
    assert attr_nl_ref.encode(np.array([5], np.uint8), 1, 1, points=one) == want7
    assert attr_nl_ref.decode(want7, one)[0].tolist() == [[6]]
    assert attr_nl_ref.lod_info(want7, 0) == attr_nl_ref.lod_info(want7, 7) == (len(want7), 1)
    assert attr_nl_ref.encode(np.zeros((0, 2), np.uint16), 2, 9, points=np.zeros((0, 3))) == bytes([ord("A"), 7, 2, 2]) + bytes(8)
    assert attr_nl_ref.info(want7) == {"version": 7, "bpv": 1, "channels": 1, "points": 1, "max_error": 1, "scalable": True, "lod": 0}
    # (c)
    pts = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 2]])
    blob = attr_nl_ref.encode(np.array([9, 12, 10], np.uint8), 1, 1, points=pts[::-1])      # any order of the rows
    assert blob[:4] == b"A\x07\x01\x01" and struct.unpack_from("<I16I", blob, 12) == (1, 3, 2) + (1,) * 14
    b2, e = attr_nl_ref._lossless_shape(blob)
    assert e == 1 and attr2_ref._residuals(b2, 3)[0][:, 0].tolist() == [3, 0, 1]
    assert attr_nl_ref.decode(blob, pts)[0][:, 0].tolist() == [9, 12, 9]
    nb, m = attr_nl_ref.lod_info(blob, 1)
    assert m == 2 and nb <= len(blob)
    assert attr_nl_ref.decode(blob[:nb], np.array([[0, 0, 1], [0, 0, 0]]), 1)[0][:, 0].tolist() == [9, 9]
    # (d)
    assert attr_ref.layout(130, 1) == (3, 1)
    v = np.zeros((130, 1), np.int64)
    v[:3, 0] = [10, 250, 0]
    j, vh = attr_nl_ref.indices4(v, 2)
    assert j[:3, 0].tolist() == [2, 48, -26] and vh[:3, 0].tolist() == [10, 250, 0]
    v[:3, 0] = [10, 254, 0]
    j, vh = attr_nl_ref.indices4(v, 7)
    assert j[:3, 0].tolist() == [1, 16, -9] and vh[:3, 0].tolist() == [15, 255, 0]
    v[:3, 0] = [3, 255, 0]
    assert attr_nl_ref.indices4(v, 7)[0][:2, 0].tolist() == [0, 17]
    v[:3, 0] = [200, 0, 0]
    j, vh = attr_nl_ref.indices4(v, 127)
    assert j[:2, 0].tolist() == [1, -1] and vh[:2, 0].tolist() == [255, 0]
    assert attr_nl_ref.decode(attr_nl_ref.encode(v, 1, 127))[0][:3, 0].tolist() == [255, 0, 0]


def test_the_entropy_stage_is_the_lossless_one():
    """the restatement's coder over the residuals of version 2 gives version 2's bytes: what differs between the lossless
    and the near-lossless kinds is what the lanes are handed, and the head"""
    rng = np.random.default_rng(5)
    pts = _grid_cloud(rng, 5000, 40, -17)
    v = _values(rng, 5000, 3, 1)
    blob = attr2_ref.encode(pts, v, 1)
    r = attr2_ref._residuals(blob, 5000)[0]
    assert blob[attr2_ref.HEAD + 64:] == attr_nl_ref._code(r, 1)
    assert attr_nl_ref.encode(v, 1, 0, points=pts) == blob and attr_nl_ref.encode(v, 1, 0) == attr_ref.encode(v, 1)


@pytest.mark.parametrize("n,c,bpv", [(1, 1, 1), (2, 4, 2), (300, 1, 1), (64 * 512 + 1, 1, 1), (3000, 3, 1), (2000, 2, 2)])
def test_restatement_round_trip_within_e(n, c, bpv):
    rng = np.random.default_rng(n + 10 * c + bpv)
    pts = _grid_cloud(rng, n, 40, -17)[rng.permutation(n)]
    v = _values(rng, n, c, bpv)                              # values at 0 and mask, alternating extremes
    mask = (1 << (8 * bpv)) - 1
    for e in (1, 2, 7, (1 << (8 * bpv - 1)) - 1):
        for scalable in (False, True):
            if scalable:
                ps, vs = _morton(pts, v)
                blob = attr_nl_ref.encode(v, bpv, e, points=pts)
                got, b = attr_nl_ref.decode(blob, pts)
            else:
                ps, vs = pts, v
                blob = attr_nl_ref.encode(v, bpv, e)
                got, b = attr_nl_ref.decode(blob)
            assert blob[1] == (7 if scalable else 4) and struct.unpack_from("<I", blob, 12)[0] == e
            assert b == bpv and got.shape == vs.shape and got.min() >= 0 and got.max() <= mask
            assert np.abs(got - vs).max() <= e, (e, scalable)
            vh = _recon(ps, vs, e, scalable)
            assert np.array_equal(got, _clip(vh, bpv)) and vh.min() >= -e and vh.max() <= mask + e, (e, scalable)
    for bad in (0, -1, 1 << (8 * bpv - 1), 1.0):
        if bad != 0:
            with pytest.raises(AssertionError):
                attr_nl_ref.encode(v, bpv, bad)


def test_restatement_rejects_a_damaged_stream():
    rng = np.random.default_rng(3)
    pts = _grid_cloud(rng, 4000, 30, 0)
    v = (np.arange(4000) * 7 % 251).astype(np.uint8)
    for kw in ({}, {"points": pts}):
        blob = bytearray(attr_nl_ref.encode(v, 1, 2, **kw))
        blob[-100] ^= 0x10
        with pytest.raises(AssertionError):
            got, _ = attr_nl_ref.decode(bytes(blob), *([pts] if kw else []))
            assert np.array_equal(got, attr_nl_ref.decode(attr_nl_ref.encode(v, 1, 2, **kw), *([pts] if kw else []))[0])


@pytest.fixture(scope="module")
def host_cases(wl):
    """name -> (points, values) in Morton order, bytes per value"""
    rng = np.random.default_rng(78)
    sweep = _unique(wl.lidar_sweep(32, 900, seed=2)["points"])
    d6 = _grid_cloud(rng, 70000, 64, 0)
    d9 = _grid_cloud(rng, 20000, 300, -30000)
    smooth = ((d6 * np.array([3, 2, 1])).sum(1)[:, None] // np.array([2, 3, 5]) + rng.integers(0, 4, (70000, 3))) % 256
    clouds = {
        "sweep 32 x 900": (sweep, wl.lidar_intensity(sweep, seed=1), 1),
        "depth 6, 3 channels": (d6, smooth, 1),
        "depth 9, uint16 x 2": (d9, _values(rng, 20000, 2, 2), 2),
        "one point": (np.array([[-7, 300, 12]], np.int32), np.array([[200, 1]]), 1),
        "empty": (np.zeros((0, 3), np.int32), np.zeros((0, 1), np.int64), 1),
    }
    out = {}
    for name, (p, v, bpv) in clouds.items():
        v = np.asarray(v, np.int64)
        out[name] = _morton(p, v[:, None] if v.ndim == 1 else v) + (bpv,)
    return out


def test_restatement_prefix_property(host_cases):
    for name, (pts, vals, bpv) in host_cases.items():
        for e in (2, 7):
            blob = attr_nl_ref.encode(vals, bpv, e, points=pts)
            full = _clip(_recon(pts, vals, e, True), bpv)
            lossless = attr2_ref.encode(pts, vals, bpv)
            prev = None
            for k in (0, 1, 2, 3, 5, 15):
                cells, want = _sample(pts, full, k)           # the reconstruction of every cell's Morton-first point
                nbytes, m = attr_nl_ref.lod_info(blob, k)
                assert m == cells.shape[0] == attr2_ref.lod_info(lossless, k)[1], (name, k)
                assert nbytes <= len(blob) and (k > 0 or nbytes == len(blob)), (name, k)
                assert prev is None or nbytes <= prev, (name, k)
                prev = nbytes
                got, b = attr_nl_ref.decode(blob[:nbytes], cells[::-1], k)
                assert b == bpv and np.array_equal(got, want), (name, e, k)
                assert m == 0 or np.abs(got - _sample(pts, vals, k)[1]).max() <= e, (name, e, k)
                if m:
                    with pytest.raises(AssertionError):
                        attr_nl_ref.decode(blob[:nbytes - 2], cells, k)


def test_attr_info_and_lod_info_against_the_restatement(host_cases):
    abi = pkg("_abi")
    GeometryCodec = pkg().GeometryCodec
    for name, (pts, vals, bpv) in host_cases.items():
        kinds = {1: attr_ref.encode(vals, bpv), 2: attr2_ref.encode(pts, vals, bpv), 4: attr_nl_ref.encode(vals, bpv, 3),
                 7: attr_nl_ref.encode(vals, bpv, 3, points=pts)}
        for ver, blob in kinds.items():
            want = attr_nl_ref.info(blob)
            assert want["version"] == ver and want["max_error"] == (3 if ver in (4, 7) and vals.shape[0] else 0)
            assert GeometryCodec.attr_info(blob) == want, (name, ver)
            assert GeometryCodec.attr_info(blob[:16]) == want, (name, ver)      # the head is enough
            if ver in (2, 7):
                for k in range(16):
                    w = attr_nl_ref.lod_info(blob, k)
                    assert GeometryCodec.attr_lod_info(blob, k) == w, (name, ver, k)
                    finer = attr_nl_ref.lod_info(blob, max(k - 1, 0))[0]
                    assert GeometryCodec.attr_lod_info(blob[:finer], k) == w, (name, ver, k)
            else:
                with pytest.raises(abi.PccError) as e:
                    GeometryCodec.attr_lod_info(blob, 1)
                assert e.value.code == abi.PCC_E_ARG, (name, ver)
    pts, vals, bpv = host_cases["depth 6, 3 channels"]
    blob = attr_nl_ref.encode(vals, bpv, 3, points=pts)
    for bad in (blob[:11], b"B" + blob[1:], b"", blob[:1] + bytes([3]) + blob[2:], blob[:1] + bytes([5]) + blob[2:],
                blob[:1] + bytes([6]) + blob[2:], blob[:2] + bytes([3]) + blob[3:], blob[:3] + bytes([5]) + blob[4:], blob[:15],
                blob[:12] + struct.pack("<I", 0) + blob[16:], blob[:12] + struct.pack("<I", 128) + blob[16:]):
        with pytest.raises(abi.PccError) as e:
            GeometryCodec.attr_info(bad)
        assert e.value.code == abi.PCC_E_STREAM, bad[:16]
    assert GeometryCodec.attr_info(blob[:12] + struct.pack("<I", 127) + blob[16:])["max_error"] == 127
    # damaged heads of version 7 through the host parse: the flip patterns of test_attr_lod_info_refusals
    nctx = attr_ref.contexts(bpv, vals.shape[1])
    for at in (0, 1, 2, 3, 8, 13, 16 + 4 * 5, 16 + 64, attr2_ref.HEAD2 + 4 + 1, attr2_ref.HEAD2 + 4 + 2 * nctx):
        bad = bytearray(blob)
        bad[at] ^= 0x55
        with pytest.raises(abi.PccError) as e:
            GeometryCodec.attr_lod_info(bytes(bad), 1)
        assert e.value.code in (abi.PCC_E_STREAM, abi.PCC_E_ARG), at
        assert e.value.code == abi.PCC_E_STREAM or at == 1, at      # another version: refused as versions 1 and 4 are


def test_compress_checks_max_error():
    check = pkg().GeometryCodec._check_max_error
    a8, a16 = np.zeros((3, 2), np.uint8), np.zeros(3, np.uint16)
    assert check(0, None) == 0 and check(0, [a8]) == 0 and check(np.int64(127), [a8, a8]) == 127 and check(32767, [a16]) == 32767
    for bad in (True, False, 1.0, "2", None, np.float32(1)):
        with pytest.raises(TypeError):
            check(bad, [a8])
    with pytest.raises(ValueError):
        check(-1, [a8])
    with pytest.raises(ValueError, match="attributes"):
        check(2, None)
    with pytest.raises(ValueError, match="frame 1:"):
        check(128, [a16, a8])
    with pytest.raises(ValueError, match="frame 0:"):
        check(32768, [a16])


def _reference_cases(wl):
    """the two reference cases of DESIGN.md 6c: the sweep's intensity and the 1M-point room's RGB, merged, Morton order"""
    sweep = wl.lidar_sweep(seed=1)["points"]
    room = wl.room(1_000_000, seed=0)
    out = {}
    for name, p, a in (("sweep intensity", sweep, wl.lidar_intensity(sweep, seed=1)),
                       ("room RGB", room["points"], np.rint(255 * room["colors"]).astype(np.uint8))):
        u, mean = attr_ref.merge(np.asarray(p, np.int32), a if a.ndim == 2 else a[:, None])
        out[name] = _morton(u, mean)
    return out


def test_rates_are_below_the_lossless_ones(wl):
    """the restatement's blobs at e = 1, 2, 4 against its lossless blobs of the same merged values (the bytes do not depend
    on the device; DESIGN.md 6d tabulates the bits per value this prints, with e = 8)"""
    for name, (pts, vals) in _reference_cases(wl).items():
        for scalable in (False, True):
            kw = {"points": pts} if scalable else {}
            sizes = {e: len(attr_nl_ref.encode(vals, 1, e, **kw)) for e in (0, 1, 2, 4, 8)}
            print(f"{name}, version {7 if scalable else 4}: " +
                  ", ".join(f"e = {e}: {b} B, {8 * b / vals.size:.2f} bits per value" for e, b in sizes.items()))
            assert sizes[0] == len(attr2_ref.encode(pts, vals, 1) if scalable else attr_ref.encode(vals, 1))
            for e in (1, 2, 4):
                assert sizes[e] < sizes[0], (name, scalable, e, sizes)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def batch(wl):
    """the mixed batch of test_geometry_attributes: the codec, the cases, the geometry blobs, the lossless attribute blobs
    of both kinds, the decoded points and the merged values in Morton order"""
    geo = pkg().GeometryCodec()
    cases = _mixed(wl)
    frames = [p for p, _ in cases]
    attrs = [a for _, a in cases]
    blobs, ab1 = geo.compress(frames, attributes=attrs)
    ab2 = geo.compress(frames, attributes=attrs, scalable=True)[1]
    pts = geo.decompress(blobs)
    want = [_expected(p, a if a.ndim == 2 else a[:, None], d) for (p, a), d in zip(cases, pts)]
    yield geo, cases, blobs, ab1, ab2, pts, want
    geo.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scalable", [False, True])
@pytest.mark.parametrize("e", ES)
def test_mixed_batch_near_lossless(batch, e, scalable):
    geo, cases, blobs, ab1, ab2, pts, want = batch
    GeometryCodec = pkg().GeometryCodec
    frames = [p for p, _ in cases]
    attrs = [a for _, a in cases]
    gb, ab = geo.compress(frames, attributes=attrs, scalable=scalable, max_error=e)
    assert gb == blobs                                                      # the geometry blobs are unaffected
    ver = 7 if scalable else 4
    got_p, got = geo.decompress(gb, ab)
    lossless = geo.decompress(gb, ab2 if scalable else ab1)[1]
    dev_p, dev = geo.decompress(gb, ab, output="device")
    for f, ((p, a), b, g) in enumerate(zip(cases, ab, got)):
        bpv = a.dtype.itemsize
        ref = attr_nl_ref.encode(want[f], bpv, e, **({"points": pts[f]} if scalable else {}))
        assert b[:2] == bytes([ord("A"), ver]) and b == ref, f"frame {f}: blob differs from the restatement's ({len(b)} vs {len(ref)} bytes)"
        info = GeometryCodec.attr_info(b)
        assert info == attr_nl_ref.info(ref) and info["max_error"] == (e if want[f].shape[0] else 0) and info["scalable"] == scalable, f
        rec = _clip(_recon(pts[f], want[f], e, scalable), bpv)
        if 0 < want[f].shape[0] <= 40000:                                   # the restatement's decoder is slow on the room
            assert np.array_equal(attr_nl_ref.decode(ref, *([pts[f]] if scalable else []))[0], rec), f
        assert g.dtype == a.dtype and g.shape == want[f].shape and np.array_equal(g, rec), f"frame {f}: decoded values differ"
        assert np.array_equal(got_p[f], pts[f]), f
        assert np.array_equal(lossless[f], want[f]), f
        err = np.abs(g.astype(np.int64) - lossless[f].astype(np.int64))
        assert err.size == 0 or err.max() <= e, f"frame {f}: off by {err.max()} from the lossless result, e = {e}"
        assert dev[f].is_cuda and np.array_equal(dev[f].cpu().numpy(), rec), f"frame {f}: device values differ"
        assert dev_p[f].is_cuda and np.array_equal(dev_p[f].cpu().numpy(), pts[f]), f
    assert len(ab[4]) == 12 and ab[4][1] == ver
    for f in (0, 1):                                                        # sweep intensity, room RGB
        assert len(ab[f]) < len((ab2 if scalable else ab1)[f]), f


@pytest.mark.gpu
def test_max_error_zero_gives_the_lossless_bytes_and_the_kinds_mix(batch):
    geo, cases, blobs, ab1, ab2, pts, want = batch
    frames = [p for p, _ in cases]
    attrs = [a for _, a in cases]
    assert geo.compress(frames, attributes=attrs, max_error=0) == (blobs, ab1)
    assert geo.compress(frames, attributes=attrs, scalable=True, max_error=0) == (blobs, ab2)
    for f, (b1, b2, w, (_, a)) in enumerate(zip(ab1, ab2, want, cases)):      # and those are the restatements' of before
        assert b1 == attr_ref.encode(w, a.dtype.itemsize) and b2 == attr2_ref.encode(pts[f], w, a.dtype.itemsize), f
    e = 2
    ab4 = geo.compress(frames, attributes=attrs, max_error=e)[1]
    ab7 = geo.compress(frames, attributes=attrs, scalable=True, max_error=e)[1]
    kinds = (ab1, ab2, ab4, ab7)
    mix = [kinds[(f + f // 4) % 4][f] for f in range(len(cases))]           # the four kinds in one call at lod 0
    assert {b[1] for b in mix} == {1, 2, 4, 7}
    for out in ("numpy", "device"):
        pm, vm = geo.decompress(blobs, mix, output=out)
        for f in range(len(cases)):
            k = (f + f // 4) % 4
            rec = want[f] if k < 2 else _clip(_recon(pts[f], want[f], e, k == 3), cases[f][1].dtype.itemsize)
            got_p, got_v = (pm[f], vm[f]) if out == "numpy" else (pm[f].cpu().numpy(), vm[f].cpu().numpy())
            assert np.array_equal(got_p, pts[f]) and got_v.dtype == cases[f][1].dtype and np.array_equal(got_v, rec), (out, f)


@pytest.mark.gpu
def test_prefixes_decode_at_a_lod(batch):
    geo, cases, blobs, ab1, ab2, pts, want = batch
    GeometryCodec = pkg().GeometryCodec
    e = 2
    frames = [p for p, _ in cases]
    attrs = [a for _, a in cases]
    ab = geo.compress(frames, attributes=attrs, scalable=True, max_error=e)[1]
    full = [_clip(_recon(p, w, e, True), a.dtype.itemsize) for p, w, (_, a) in zip(pts, want, cases)]
    for k in (1, 2, 3, 4):
        direct = [_sample(p, w, k) for p, w in zip(pts, full)]              # the reconstruction of every cell's first point
        exact = [_sample(p, w, k)[1] for p, w in zip(pts, want)]
        ginfo = [GeometryCodec.lod_info(b, k) for b in blobs]
        ainfo = [GeometryCodec.attr_lod_info(a, k) for a in ab]
        for f, (g, a) in enumerate(zip(ginfo, ainfo)):
            assert g[1] == a[1] == direct[f][0].shape[0] and a == attr_nl_ref.lod_info(ab[f], k), (k, f)
        gpre = [b[:n] for b, (n, _) in zip(blobs, ginfo)]
        apre = [a[:n] for a, (n, _) in zip(ab, ainfo)]
        for what, gs, as_ in (("the two shortest prefixes", gpre, apre), ("whole blobs", blobs, ab)):
            cells, vals = geo.decompress(gs, as_, lod=k)
            dcells, dvals = geo.decompress(gs, as_, output="device", lod=k)
            for f, (wc, wv) in enumerate(direct):
                assert isinstance(vals[f], np.ndarray) and vals[f].dtype == cases[f][1].dtype, (k, what, f)
                assert np.array_equal(cells[f], wc), f"lod {k}, {what}, frame {f}: cells differ"
                assert vals[f].shape == wv.shape and np.array_equal(vals[f], wv), f"lod {k}, {what}, frame {f}: values differ"
                assert wv.size == 0 or np.abs(vals[f].astype(np.int64) - exact[f]).max() <= e, (k, what, f)
                assert dvals[f].is_cuda and np.array_equal(dvals[f].cpu().numpy(), wv), f"lod {k}, {what}, frame {f}: device values"
                if what != "whole blobs" and 0 < wv.shape[0] <= 40000:
                    assert np.array_equal(attr_nl_ref.decode(apre[f], wc, k)[0], wv), (k, f)


@pytest.mark.gpu
def test_compress_scalable_at_a_lod_with_e(batch, wl):
    """the sender's side: compress(..., lod=k, scalable=True, max_error=e) codes the cells' means over the cells' keys"""
    geo = batch[0]
    rng = np.random.default_rng(6)
    sweep = wl.lidar_sweep(32, 900, seed=5)["points"]
    dup = np.concatenate([sweep[:4000], sweep[:900]])
    cases = [(sweep, wl.lidar_intensity(sweep, seed=1)), (np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint16)),
             (dup, rng.integers(0, 65536, (dup.shape[0], 3)).astype(np.uint16))]
    e = 4
    for k in (1, 3):
        for scalable in (True, False):
            gb, ab = geo.compress([p for p, _ in cases], attributes=[a for _, a in cases], lod=k, scalable=scalable, max_error=e)
            assert gb == geo.compress([p for p, _ in cases], lod=k)
            cells, got = geo.decompress(gb, ab)
            for f, (p, a) in enumerate(cases):
                u, mean = attr_ref.merge(np.asarray(p, np.int32) >> k, a if a.ndim == 2 else a[:, None])
                us, ms = _morton(u + (32768 >> k) - 32768, mean)          # Morton order under the bias 32768 >> k
                assert np.array_equal(cells[f], us + 32768 - (32768 >> k)), (k, f)
                if not scalable:
                    assert ab[f] == attr_nl_ref.encode(ms, a.dtype.itemsize, e), (k, f)
                    assert np.array_equal(got[f], _clip(attr_nl_ref.indices4(ms, e)[1] if ms.size else ms, a.dtype.itemsize)), (k, f)
                    continue
                assert ab[f] == attr_nl_ref.encode(mean, a.dtype.itemsize, e, points=u, bias=32768 >> k), (k, f)
                assert pkg().GeometryCodec.attr_info(ab[f])["lod"] == k
                if ms.size:
                    s, _, first = attr2_ref.intro(attr2_ref.keys_of(us))
                    rec = _clip(attr_nl_ref.indices7(ms, s, first, e)[1], a.dtype.itemsize)
                    assert np.array_equal(got[f], rec) and np.abs(rec - ms).max() <= e, (k, f)
                    c2, v2 = geo.decompress([gb[f]], [ab[f][:geo.attr_lod_info(ab[f], 2)[0]]], lod=2)
                    wc, wv = _sample(us, rec, 2)
                    assert np.array_equal(v2[0], wv) and c2[0].shape[0] == wc.shape[0], (k, f)


@pytest.mark.gpu
def test_float32_device_frames_drop_and_index_with_e(batch, wl):
    import torch
    geo = batch[0]
    rng = np.random.default_rng(12)
    voxel, origin = 0.05, (1.0, -2.0, 0.5)
    lats = [wl.lidar_sweep(32, 900, seed=7)["points"].astype(np.int32), random_cloud(rng, 3000, extent=100, lo=-50)[:, 1:]]
    lats[1] = np.concatenate([lats[1], lats[1][:500]])                      # duplicates
    attrs = [wl.lidar_intensity(lats[0], seed=3), rng.integers(0, 65536, (3500, 2)).astype(np.uint16)]
    fl = [(p.astype(np.float32) * np.float32(voxel) + np.asarray(origin, np.float32)).astype(np.float32) for p in lats]
    e = 2
    for scalable in (False, True):
        want = geo.compress(lats, attributes=attrs, scalable=scalable, max_error=e, return_index=True)
        plain = geo.compress(lats, attributes=attrs, scalable=scalable, return_index=True)
        assert want[0] == plain[0] and all(np.array_equal(x, y) for x, y in zip(want[2], plain[2]))
        assert all(b[1] == (7 if scalable else 4) for b in want[1])
        got = geo.compress(fl, attributes=attrs, scalable=scalable, max_error=e, voxel=voxel, origin=origin, return_index=True)
        assert got[0] == want[0] and got[1] == want[1] and all(np.array_equal(x, y) for x, y in zip(got[2], want[2])), scalable
        dev = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in fl], attributes=attrs, scalable=scalable, max_error=e,
                           voxel=voxel, origin=origin, return_index=True)
        assert dev[0] == want[0] and dev[1] == want[1], scalable
        assert all(i.is_cuda and np.array_equal(i.cpu().numpy(), w) for i, w in zip(dev[2], want[2])), scalable
        dint = geo.compress([torch.from_numpy(p).to(geo.rt.device) for p in lats], attributes=attrs, scalable=scalable, max_error=e)
        assert dint == (want[0], want[1]), scalable
        # rows without a return are dropped before coding: the blobs of the kept rows
        holes = [f.copy() for f in fl]
        valid = []
        for f in holes:
            rows = rng.permutation(f.shape[0])[:f.shape[0] // 10]
            f[rows, rng.integers(0, 3, rows.size)] = np.nan
            valid.append(np.isfinite(f).all(axis=1))
        holes.append(np.full((5, 3), np.nan, np.float32))
        valid.append(np.zeros(5, bool))
        hattrs = attrs + [np.arange(5, dtype=np.uint8)]
        kept = geo.compress([f[v] for f, v in zip(holes, valid)], attributes=[a[v] for a, v in zip(hattrs, valid)],
                            scalable=scalable, max_error=e, voxel=voxel, origin=origin)
        for put in (lambda fs: fs, lambda fs: [torch.from_numpy(f).to(geo.rt.device) for f in fs]):
            drop = geo.compress(put(holes), attributes=hattrs, scalable=scalable, max_error=e, voxel=voxel, origin=origin,
                                invalid="drop")
            assert drop == kept, scalable
        assert len(kept[1][2]) == 12 and kept[1][2][1] == (7 if scalable else 4)
        pts, vals = geo.decompress(want[0], want[1], voxel=voxel, origin=origin)
        exact = geo.decompress(plain[0], plain[1])[1]
        assert all(p.dtype == np.float32 for p in pts)
        assert all(np.abs(a.astype(np.int64) - b.astype(np.int64)).max() <= e for a, b in zip(vals, exact)), scalable


@pytest.mark.gpu
def test_argument_checks_of_compress(batch):
    abi = pkg("_abi")
    geo, cases = batch[0], batch[1]
    p, a = cases[3]
    for bad in (True, 1.5, "1"):
        with pytest.raises(TypeError):
            geo.compress([p], attributes=[a], max_error=bad)
    with pytest.raises(ValueError):
        geo.compress([p], attributes=[a], max_error=-1)
    with pytest.raises(ValueError, match="attributes"):
        geo.compress([p], max_error=1)
    with pytest.raises(ValueError, match="frame 1:"):
        geo.compress([cases[2][0], p], attributes=[cases[2][1], a], max_error=128)      # uint16, then uint8
    gb, ab = geo.compress([cases[2][0], p], attributes=[cases[2][1], a], max_error=127)
    assert [pkg().GeometryCodec.attr_info(b)["max_error"] for b in ab] == [127, 127]
    got = geo.decompress(gb, ab)[1]
    exact = geo.decompress(*geo.compress([cases[2][0], p], attributes=[cases[2][1], a]))[1]
    assert all(np.abs(x.astype(np.int64) - y.astype(np.int64)).max() <= 127 for x, y in zip(got, exact))
    gb, ab = geo.compress([cases[2][0]], attributes=[cases[2][1]], max_error=32767, scalable=True)
    got = geo.decompress(gb, ab)[1][0]
    assert np.abs(got.astype(np.int64) - exact[0].astype(np.int64)).max() <= 32767
    # the C entry point refuses what the Python layer would have caught
    with pytest.raises(abi.PccError) as e:
        with geo._lock, geo.rt as rt:
            rt.attr_encode_frames(None, [0], [1 | (1 << 8)], [0, 0], [0], None, None, 0, 1, max_error=128)
    assert e.value.code == abi.PCC_E_ARG and "frame 0:" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("scalable", [False, True])
def test_corrupt_blobs_are_named_and_the_codec_stays_usable(batch, scalable):
    """the flip patterns of test_geometry_attributes (bit i % 8 of every head byte, 0x21 into payload bytes, cuts) on the
    c = 4 frame of a run of six.  Every head byte must be refused except: the lowest byte of max_error, where a flip
    gives another valid e (the header itself is then well formed, and only the range check of the reconstructions can
    notice), and the initial probabilities p0, where a flip moves one slot of one context's interval (as
    test_geometry_attributes_lod says of them); there a result of the right shape may come back."""
    abi = pkg("_abi")
    geo, cases, blobs, ab1, ab2, pts, want = batch
    e = 2
    k = 3                                                                   # the c = 4 frame
    sub_g = blobs[2:8]
    sub_a = geo.compress([p for p, _ in cases[2:8]], attributes=[a for _, a in cases[2:8]], scalable=scalable, max_error=e)[1]
    good = geo.decompress(sub_g, sub_a)[1]
    kk = k - 2
    b = sub_a[kk]
    nctx = attr_ref.contexts(1, 4)
    p0_at = (attr2_ref.HEAD2 if scalable else attr_ref.HEAD + 8) + 4
    head = p0_at + 2 * nctx + 4                                             # one chunk
    assert struct.unpack_from("<I", b, p0_at - 4)[0] == 1 and b[1] == (7 if scalable else 4)

    def swapped(nb):
        return sub_a[:kk] + [bytes(nb)] + sub_a[kk + 1:]
    bad = {f"header byte {i}": b[:i] + bytes([b[i] ^ (1 << (i % 8))]) + b[i + 1:] for i in range(head)}
    rng = np.random.default_rng(11)
    for i in sorted(set(rng.integers(head, len(b), 16).tolist()) | {head, head + 300, head + 700, len(b) // 2, len(b) - 3, len(b) - 1}):
        bad[f"payload byte {i}"] = b[:i] + bytes([b[i] ^ 0x21]) + b[i + 1:]
    bad["cut"] = b[:-2]
    bad["cut header"] = b[:15]
    bad["cut behind max_error"] = b[:16]
    bad["max_error 0"] = b[:12] + struct.pack("<I", 0) + b[16:]
    bad["max_error 128"] = b[:12] + struct.pack("<I", 128) + b[16:]
    lenient = {f"header byte {i}" for i in range(p0_at, p0_at + 2 * nctx)} | {"header byte 12"}
    for what, nb in bad.items():
        try:
            got = geo.decompress(sub_g, swapped(nb))[1]
        except abi.PccError as err:
            assert f"frame {kk}:" in str(err), (what, str(err))
        else:
            assert what in lenient, f"{what}: not refused"
            assert got[kk].shape == good[kk].shape, what
        again = geo.decompress(sub_g, sub_a)[1]                             # the next call on the same instance
        assert all(np.array_equal(x, y) for x, y in zip(again, good)), what
    # an attribute blob beside the geometry of a frame with another point count
    with pytest.raises(abi.PccError) as err:
        geo.decompress(sub_g, sub_a[:1] + [sub_a[2], sub_a[1]] + sub_a[3:])
    assert err.value.code == abi.PCC_E_STREAM and "frame 1:" in str(err.value)
    if scalable:                                                            # a prefix at lod 1: heads and a cut
        GeometryCodec = pkg().GeometryCodec
        gpre = [g[:GeometryCodec.lod_info(g, 1)[0]] for g in sub_g]
        apre = [a[:GeometryCodec.attr_lod_info(a, 1)[0]] for a in sub_a]
        good1 = geo.decompress(gpre, apre, lod=1)[1]
        pre = apre[kk]
        for what, nb in [(f"header byte {i}", pre[:i] + bytes([pre[i] ^ (1 << (i % 8))]) + pre[i + 1:]) for i in range(p0_at)] + \
                [("two bytes short", pre[:-2]), ("cut header", pre[:40])]:
            try:
                got = geo.decompress(gpre, apre[:kk] + [nb] + apre[kk + 1:], lod=1)[1]
            except abi.PccError as err:
                assert f"frame {kk}:" in str(err), (what, str(err))
                assert "truncated" in str(err) or what != "two bytes short", (what, str(err))
            except ValueError as err:
                raise AssertionError(f"{what}: {err}")
            else:
                assert what == "header byte 12" and got[kk].shape == good1[kk].shape, f"{what}: not refused"
            again = geo.decompress(gpre, apre, lod=1)[1]
            assert all(np.array_equal(x, y) for x, y in zip(again, good1)), what


@pytest.mark.gpu
def test_kinds_are_refused_where_they_do_not_belong(batch):
    abi = pkg("_abi")
    geo, cases, blobs, ab1, ab2, pts, want = batch
    GeometryCodec = pkg().GeometryCodec
    p, a = cases[2]
    gb, ab4 = geo.compress([p], attributes=[a], max_error=3)
    ab7 = geo.compress([p], attributes=[a], max_error=3, scalable=True)[1]
    with pytest.raises(ValueError, match="version 4"):                     # version 4 has no levels of detail
        geo.decompress(gb, ab4, lod=1)
    with pytest.raises(ValueError, match="attribute"):
        geo.decompress([gb[0], gb[0]], [ab7[0], ab4[0]], lod=1)
    with pytest.raises(abi.PccError) as e:
        GeometryCodec.attr_lod_info(ab4[0], 1)
    assert e.value.code == abi.PCC_E_ARG
    assert GeometryCodec.attr_lod_info(ab7[0], 0) == (len(ab7[0]), GeometryCodec.attr_info(ab7[0])["points"])
    with geo._lock, geo.rt as rt:
        cells = rt.octree_decode_frames(gb, device=True, lod=0)
        cells2 = rt.octree_decode_frames([gb[0], gb[0]], device=True, lod=0)
        for blobs_, kw, code in (([ab7[0]], {}, abi.PCC_E_STREAM),                       # the lod entry point's kinds
                                 ([ab2[2]], {}, abi.PCC_E_STREAM),
                                 ([ab4[0]], {"lod": 0, "cells": cells}, abi.PCC_E_STREAM),      # and the other's
                                 ([ab1[2]], {"lod": 0, "cells": cells}, abi.PCC_E_STREAM),
                                 ([ab1[2], ab4[0]], {}, abi.PCC_E_ARG),                  # one version per call
                                 ([ab4[0], ab1[2]], {}, abi.PCC_E_ARG),
                                 ([ab2[2], ab7[0]], {"lod": 0, "cells": cells2}, abi.PCC_E_ARG),
                                 ([ab7[0], ab2[2]], {"lod": 0, "cells": cells2}, abi.PCC_E_ARG)):
            with pytest.raises(abi.PccError) as e:
                rt.attr_decode_frames(blobs_, **kw)
            assert e.value.code == code and ("frame 0:" in str(e.value) or "frame 1:" in str(e.value)), (kw, str(e.value))
    for ver in (3, 5, 6):                                                   # the other version bytes stay refused
        for src in (ab4[0], ab7[0]):
            with pytest.raises(abi.PccError) as e:
                geo.decompress(gb, [src[:1] + bytes([ver]) + src[2:]])
            assert "frame 0:" in str(e.value), ver
    got = geo.decompress([gb[0], gb[0]], [ab4[0], ab7[0]])[1]               # and the codec stays usable
    assert np.abs(got[0].astype(np.int64) - want[2]).max() <= 3 and np.abs(got[1].astype(np.int64) - want[2]).max() <= 3
