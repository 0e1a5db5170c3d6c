"""Transform-coded attribute blobs with level-of-detail prefixes, version 22 (include/pcc.h has the rule), on the host:
a blob worked by hand in which both weight regimes occur, the numpy restatement tests/attr_scalable_ref.py through its
own decoder at the rule's edges and at every cut, the property the kind exists for (a decoder at a cut reproduces what
the full inverse holds there), the shortest prefixes, bytes and error beside version 19 on the 25 recorded frames, the
host-only entry points with what they refuse, and what compress refuses before it enters the runtime.  No GPU."""
import os
import struct

import numpy as np
import pytest

import attr2_ref
import attr_colour_ref as C21
import attr_ref
import attr_scalable_ref as S
import attr_transform_ref as T
from conftest import ROOT, pkg, random_cloud
from test_geometry_attributes_lod import _morton

GeometryCodec = pkg().GeometryCodec


def _cloud(rng, n, extent=60):
    pts = random_cloud(rng, n, extent=extent, lo=-extent // 2)[:, 1:]
    return pts[np.argsort(attr2_ref.keys_of(pts))]                          # Morton order: row i of the values is point i


def _smooth(rng, n, c, bpv):
    top = 1 << (8 * bpv)
    base = np.cumsum(rng.integers(-9, 10, n)) * (1 if bpv == 1 else 97) + rng.integers(0, top)
    return ((base[:, None] + rng.integers(-4, 5, (n, c)) * (1 if bpv == 1 else 50)) % top).astype(np.int64)


def _cells(pts, j):
    c = np.asarray(pts, np.int64) >> j
    _, first = np.unique(attr2_ref.keys_of(c), return_index=True)
    return c[first]


def test_a_blob_worked_by_hand():
    """three points A = (0, 0, 0), B = (0, 0, 1), C = (0, 0, 2) with values 10, 20, 50, one channel, q = 4, K = 1.
    b(B) = 0 (inside A's 1-cell), b(C) = 3 = 3 K (two 1-cells).  first = A, C: g = 0, 1, 1, 2; C = 2;
    M = max(1, floor((6 + 2) / 4)) = 2.
    t = 0, pair B | lo = A: h = 10, val[A] = 10 + floor(10 / 2) = 15, s = max(2, isqrt(floor(2 * 16 / 2^0))) = 5,
                            x[B] = floor((10 + 2) / 5) = 2
    t = 3, pair C | lo = A, hi = 3: ca = 1, cb = 1, w = 2, h = 50 - 15 = 35, val[A] = 15 + floor(1 * 35 / 2) = 32,
                            s = max(2, isqrt(floor(16 * 2 / (1 * 1 * 2)))) = 4, x[C] = floor((35 + 2) / 4) = 9
    x[A] = 32 - 128 = -96.  Coding order A, C, B: -96, 9, 2.
    Inverse: val[A] = 32; t = 3: h^ = 36, val[A] = 32 - 18 = 14, val[C] = 50; t = 0: h^ = 10, val[A] = 14 - 5 = 9,
    val[B] = 19.  At the cut j = 1 the cells are {A, B} and {C} and the coefficients -96, 9: 14 and 50, what the full
    inverse holds at A and C behind sublevel 3."""
    pts = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 2]])
    vals = np.array([[10], [20], [50]])
    keys = attr2_ref.keys_of(pts)
    assert T.sublevels(keys).tolist() == [48, 0, 3]
    assert S.kcells(keys, 0, 1).tolist() == [0, 1, 1, 2] and S.scale(3, 2) == 2
    x = S.forward(keys, vals, 4, 1, 1)
    assert x[:, 0].tolist() == [-96, 2, 9]
    blob = S.encode(pts, vals, 1, 4, 1)
    head = bytes([ord("A"), 22, 1, 1]) + struct.pack("<II", 3, len(blob) - 12) + struct.pack("<III", 0, 4, 1)
    head += struct.pack("<16I", 3, 2, *([1] * 14)) + struct.pack("<II", 1, 1)
    assert blob[:len(head)] == head and len(head) == 12 + 4 + 4 + 4 + 64 + 8
    assert S.indices(blob, 3)[:, 0].tolist() == [-96, 9, 2]
    assert S.decode(blob, pts)[0][:, 0].tolist() == [9, 19, 50]
    nbytes, m = S.lod_info(blob, 1)
    assert m == 2 and nbytes <= len(blob)
    assert S.decode(blob[:nbytes], np.array([[0, 0, 0], [0, 0, 1]]), 1)[0][:, 0].tolist() == [14, 50]
    assert S.stopped(keys, x, 4, 1, 1, 1)[:, 0].tolist() == [14, 50]
    assert GeometryCodec.attr_info(blob) == S.info(blob)
    assert GeometryCodec.attr_lod_info(blob, 1) == (nbytes, 2) and GeometryCodec.attr_lod_info(blob, 0) == (len(blob), 3)


EDGES = [  # n, extent, c, bpv, q, K, colour, slod
    (1, 60, 3, 1, 7, 1, 1, 0), (2, 60, 1, 1, 7, 3, 0, 0), (2, 4, 3, 1, 7, 15, 1, 0), (200, 60, 3, 1, 1, 2, 0, 0),
    (200, 60, 3, 1, 127, 2, 1, 0), (250, 8, 3, 1, 9, 3, 1, 0), (250, 60, 4, 2, (900, 1500, 2000, 5), 2, 1, 0),
    (250, 60, 2, 2, (32767, 1), 1, 0, 0), (200, 60, 3, 1, 12, 5, 0, 10), (40, 4, 3, 1, 12, 1, 1, 14)]


@pytest.mark.parametrize("case", EDGES, ids=[f"n{c[0]}-e{c[1]}-c{c[2]}-b{c[3]}-K{c[5]}-s{c[7]}" for c in EDGES])
def test_round_trips_at_every_cut(case):
    """decode(encode) at every lod 0 .. K from lod_info's prefix is the restatement's reconstruction there and the full
    inverse stopped behind sublevel 3 lod (clamped and colour-inverted); one byte less does not decode"""
    n, extent, c, bpv, q, K, colour, slod = case
    rng = np.random.default_rng(n + 7 * K + c)
    pts = _cloud(rng, n, extent)
    if extent == 8:
        pts = pts + 4 + 64                                                  # one 8 x 8 x 8 cell: no pair at or above 3 K
    vals = _smooth(rng, pts.shape[0], c, bpv)
    bias = 32768 >> slod
    blob = S.encode(pts, vals, bpv, q, K, colour, bias)
    assert blob[1] == 22 and blob[2] == bpv | (slod << 4)
    i = S.info(blob)
    assert (i["scalable_to"], i["scalable"], i["lod"], i["points"]) == (K, True, slod, pts.shape[0])
    keys, v = T._sorted(pts, vals, bias)
    if colour:
        v = C21.colour_forward(v, bpv)
    x = S.forward(keys, v, q, bpv, K)
    for j in range(K + 1):
        cells = _cells(pts, j)
        nbytes, m = S.lod_info(blob, j)
        assert m == cells.shape[0] and (j > 0 or nbytes == len(blob))
        got = S.decode(blob[:nbytes], cells, j)[0]
        assert np.array_equal(got, S.reconstruct(pts, vals, bpv, q, K, colour, bias, lod=j)), j
        stop = np.clip(S.stopped(keys, x, q, bpv, K, j), 0, (1 << (8 * bpv)) - 1)
        assert np.array_equal(got, C21.colour_inverse(stop, bpv) if colour else stop), j
        with pytest.raises(AssertionError):
            S.decode(blob[:nbytes - 1], cells, j)
        if j and n >= 100:
            assert S.lod_info(blob[:nbytes - 1], j) == (nbytes, m)          # the plan needs the length table only
    with pytest.raises(AssertionError):
        S.lod_info(blob, K + 1)
    if slod + K < 15 and pts.shape[0] > 1:
        with pytest.raises(AssertionError):
            S.decode(blob, _cells(pts, K + 1), K + 1)


def test_empty_frame_and_the_rules_refusals():
    assert S.encode(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), 1, 5, 2, 1) == bytes([ord("A"), 22, 1, 3]) + bytes(8)
    pts, vals = _cloud(np.random.default_rng(1), 50, 10), _smooth(np.random.default_rng(2), 50, 3, 1)
    for K, bias in ((0, 32768), (16, 32768), (True, 32768), (6, 32768 >> 10), (1.0, 32768)):
        with pytest.raises(AssertionError):
            S.encode(pts, vals, 1, 5, K, 0, bias)
    blob = S.encode(pts, vals, 1, 5, 2)
    other = _cloud(np.random.default_rng(3), 50, 12)                         # as many points, another number of K-cells
    assert S.kcells(attr2_ref.keys_of(other), 0, 2)[-1] != S.kcells(attr2_ref.keys_of(pts), 0, 2)[-1]
    with pytest.raises(AssertionError):
        S.decode(blob, other)


@pytest.mark.parametrize("colour", [0, 1])
def test_a_decoder_at_a_cut_sees_what_the_full_inverse_holds_there(colour):
    """the property the weights were chosen for, on recorded frames 0 and 12: for every j <= K = 3 a decoder that sees the
    cells of lod j and the first count[j] coefficients reproduces, value for value, what the full inverse holds at the
    first leaf of every cell behind sublevel 3 j"""
    for i in (0, 12):
        pts, vals = _zed(i)
        vals = np.asarray(vals, np.int64)
        keys, v = T._sorted(pts, vals, 32768)
        if colour:
            v = C21.colour_forward(v, 1)
        x = S.forward(keys, v, 32, 1, 3)
        b = T.sublevels(keys)
        g = S.kcells(keys, 0, 3)
        for j in range(4):
            kappa = keys[b >= 3 * j] >> np.uint64(3 * j)
            cut = S.inverse(kappa, x[b >= 3 * j], 32, 1, 3, j, keys.shape[0], int(g[-1]), clamp=False)
            assert np.array_equal(cut, S.stopped(keys, x, 32, 1, 3, j)), (i, j)


def _zed(i):
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        u, mean = attr_ref.merge(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"])
    return _morton(u, mean)


# What the prefixes cost on recorded camera colour (RGB, no colour transform), measured with the restatements on all 25
# frames of tests/golden/zed_seq25.npz (16098 .. 21277 points): whole blobs in bytes summed over the frames, the mean of
# the frames' MSE, and per frame the ratios to version 19 at the same q.
#
#   q    kind        bytes    MSE     bytes / v19       MSE / v19
#   16   version 19  328722   17.41
#   16   K = 1       334830   17.94   1.003 .. 1.030    0.935 .. 1.141
#   16   K = 2       358938   16.29   1.074 .. 1.107    0.807 .. 1.085
#   16   K = 3       370584   15.07   1.107 .. 1.146    0.750 .. 1.007
#   32   version 19  209722   46.47
#   32   K = 1       215516   48.14   1.006 .. 1.042    0.974 .. 1.106
#   32   K = 2       237082   41.88   1.105 .. 1.149    0.821 .. 0.977
#   32   K = 3       246946   38.64   1.148 .. 1.197    0.780 .. 0.884
#
# The asserted margin per (K, q) is the worst ratio over the 25 frames plus a tenth of it, for bytes and for MSE, so
# that a later change to the rule that costs rate or error shows: (bytes bound, MSE bound)
RATE_BOUND = {(1, 16): (1.134, 1.256), (2, 16): (1.218, 1.194), (3, 16): (1.261, 1.108),
              (1, 32): (1.147, 1.217), (2, 32): (1.265, 1.075), (3, 32): (1.317, 0.972)}


def test_rate_and_error_beside_version_19_on_the_recorded_frames():
    worst = {k: [0.0, 0.0] for k in RATE_BOUND}
    for i in range(25):
        pts, vals = _zed(i)
        vals = np.asarray(vals, np.int64)
        for q in (16, 32):
            t_bytes = len(T.encode(pts, vals, 1, q))
            t_mse = float(((T.reconstruct(pts, vals, 1, q) - vals) ** 2).mean())
            line = f"frame {i} ({len(pts)} points) q={q}: version 19 {t_bytes} B, mse {t_mse:.1f}"
            for K in (1, 2, 3):
                s_bytes = len(S.encode(pts, vals, 1, q, K))
                s_mse = float(((S.reconstruct(pts, vals, 1, q, K) - vals) ** 2).mean())
                line += f"; K={K} {s_bytes} B, mse {s_mse:.1f}"
                worst[K, q] = [max(worst[K, q][0], s_bytes / t_bytes), max(worst[K, q][1], s_mse / t_mse)]
                assert s_bytes <= RATE_BOUND[K, q][0] * t_bytes and s_mse <= RATE_BOUND[K, q][1] * t_mse, (i, K, q, line)
            print(line)
    print("worst ratios (bytes, mse):", {k: (round(v[0], 4), round(v[1], 4)) for k, v in worst.items()})


def test_host_parse_and_refusals():
    """pcc_attr_info, pcc_attr_transform_info, pcc_attr_scalable_to and pcc_attr_lod_info on version 22: what they read
    back, from the blob and from prefixes, and what they refuse"""
    abi = pkg("_abi")
    rng = np.random.default_rng(3)
    pts = _cloud(rng, 300)
    vals = _smooth(rng, 300, 3, 1)
    blob = S.encode(pts, vals, 1, (5, 11, 12), 3, 1)
    want = {"version": 22, "bpv": 1, "channels": 3, "points": 300, "qstep": (5, 11, 12), "colour": "ycocg", "max_error": 0,
            "scalable": True, "scalable_to": 3, "lod": 0}
    assert GeometryCodec.attr_info(blob) == want == S.info(blob)
    reach, head = 20 + 4 * 3, 12 + 4 + 12 + 4 + 64 + 8
    for cut in (reach, reach + 1, head - 1, head, head + 100, head + 2 * 240 + 2, len(blob) - 1):
        assert GeometryCodec.attr_info(blob[:cut]) == want, cut
    for j in range(4):
        assert GeometryCodec.attr_lod_info(blob, j) == S.lod_info(blob, j), j
        nbytes = S.lod_info(blob, j)[0]
        assert GeometryCodec.attr_lod_info(blob[:nbytes], j)[0] == nbytes
    cells = np.unique(pts >> 3, axis=0)
    b16 = S.encode(cells, _smooth(rng, cells.shape[0], 4, 2), 2, (32767, 1, 2, 3), 12, 1, 32768 >> 3)
    i16 = GeometryCodec.attr_info(b16)
    assert i16 == S.info(b16) and (i16["bpv"], i16["channels"], i16["scalable_to"], i16["lod"]) == (2, 4, 12, 3)
    empty = bytes([ord("A"), 22, 1 | (15 << 4), 4]) + bytes(8)
    assert GeometryCodec.attr_info(empty) == {"version": 22, "bpv": 1, "channels": 4, "points": 0, "qstep": (0, 0, 0, 0), "colour": None,
                                              "max_error": 0, "scalable": True, "scalable_to": 0, "lod": 15} == S.info(empty)
    assert GeometryCodec.attr_lod_info(empty, 9) == (12, 0)
    # the other kinds' dicts are unchanged, and pcc_attr_scalable_to says 0 for them
    import ctypes as C
    b21 = C21.encode(pts, vals, 1, (5, 11, 12), 1)
    assert GeometryCodec.attr_info(b21) == C21.info(b21) and "scalable_to" not in GeometryCodec.attr_info(b21)
    buf = np.frombuffer(b21, np.uint8)
    k = C.c_int32(-1)
    assert abi.lib().pcc_attr_scalable_to(C.c_void_p(buf.ctypes.data), len(b21), C.byref(k)) == 0 and k.value == 0

    def refused(bad, code=abi.PCC_E_STREAM, lod=None):
        with pytest.raises(abi.PccError) as e:
            GeometryCodec.attr_info(bad) if lod is None else GeometryCodec.attr_lod_info(bad, lod)
        assert e.value.code == code, (bad[:16], str(e.value))

    def patched(at, fmt, *v, of=blob):
        return of[:at] + struct.pack(fmt, *v) + of[at + struct.calcsize(fmt):]
    at_k = 16 + 12
    for K in (0, 16, 1 << 31):                                              # K = 0, and slod + K > 15
        refused(patched(at_k, "<I", K))
        refused(patched(at_k, "<I", K)[:reach])
        refused(patched(at_k, "<I", K), lod=0)
    refused(patched(16 + 4 * 4, "<I", 13, of=b16))                                # 3 + 13 > 15
    assert GeometryCodec.attr_info(patched(16 + 4 * 4, "<I", 11, of=b16))["scalable_to"] == 11
    refused(blob, abi.PCC_E_ARG, lod=4)                                     # above K
    refused(blob, abi.PCC_E_ARG, lod=15)
    refused(blob[:reach - 1])                                               # K is cut
    refused(blob[:head], lod=1)                                             # no chunk table to plan from
    refused(patched(12, "<I", 2))                                           # a colour word above 1
    for ch in range(3):
        refused(patched(16 + 4 * ch, "<I", 0))                              # a step of 0, of H
        refused(patched(16 + 4 * ch, "<I", 128)[:reach])
    counts = at_k + 4
    refused(patched(counts, "<I", 301))                                     # count[0] is not n
    refused(patched(counts + 8, "<I", struct.unpack_from("<I", blob, counts + 4)[0] + 1))      # a level that grows
    refused(patched(counts + 4, "<I", 300 // 9))                            # a level below an eighth of the one before
    refused(patched(counts + 60, "<I", 0), lod=2)
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
    refused(patched(head, "<H", 5000))                                      # an initial probability out of range
    refused(bytes([ord("A"), 22, 1, 3]) + struct.pack("<II", 0, 4) + bytes(4))      # no points, a payload
    for other in (20, 23, 6, 18, 54, 0x96):                                 # neighbours of 22 are no kind
        refused(patched(1, "B", other))
    # versions 19 and 21 keep their refusal
    refused(b21, abi.PCC_E_ARG, lod=0)
    refused(T.encode(pts, vals, 1, 32), abi.PCC_E_ARG, lod=1)


def test_byte_22_against_the_rule_of_the_version_bytes():
    """odd parity, so two bits from each of the other ten"""
    kinds = (1, 2, 4, 7, 8, 11, 13, 14, 19, 21)
    assert bin(22).count("1") % 2 == 1 and all(bin(k).count("1") % 2 == 1 for k in kinds)
    assert all(bin(22 ^ k).count("1") >= 2 for k in kinds)


def test_abi_is_declared_and_bound():
    abi = pkg("_abi")
    with open(os.path.join(ROOT, "include", "pcc.h")) as f:
        text = f.read()
    for name in ("pcc_attr_encode_frames_transform3", "pcc_attr_scalable_to"):
        assert name in abi.PROTOTYPES and name + "(" in text, name
        assert getattr(abi.lib(), name) is not None


def test_compress_checks_scalable_to():
    """the checks of compress that run before the runtime is entered: on an instance that has none"""
    geo = object.__new__(GeometryCodec)
    pts = [np.zeros((3, 3), np.int32) + np.arange(3, dtype=np.int32)[:, None]] * 2
    a8, a84 = np.zeros((3, 3), np.uint8), np.zeros((3, 4), np.uint8)
    for bad in (True, False, 1.0, "2", (2,), np.float32(2)):
        with pytest.raises(TypeError, match="scalable_to"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, scalable_to=bad)
    for bad, lod in ((0, 0), (-1, 0), (16, 0), (15, 1), (6, 10)):
        with pytest.raises(ValueError, match=f"scalable_to must be an integer in 1 .. {15 - lod}"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, scalable_to=bad, lod=lod)
    with pytest.raises(ValueError, match="it needs qstep="):
        geo.compress(pts, attributes=[a8, a8], scalable_to=2)
    with pytest.raises(ValueError, match="it needs qstep="):
        geo.compress(pts, attributes=[a8, a8], qstep=0, scalable_to=2)
    with pytest.raises(ValueError, match="it needs qstep="):
        geo.compress(pts, scalable_to=2)
    for kw in (dict(max_error=1), dict(cross_channel=True), dict(scalable=True)):
        with pytest.raises(ValueError, match="scalable_to with max_error, cross_channel or scalable=True"):
            geo.compress(pts, attributes=[a8, a8], scalable_to=2, **kw)
    # beside qstep the three keep the message they had
    with pytest.raises(ValueError, match="scalable=True: a transform-coded blob"):
        geo.compress(pts, attributes=[a8, a8], qstep=4, scalable=True, scalable_to=2)
    with pytest.raises(ValueError, match="max_error: a transform-coded blob"):
        geo.compress(pts, attributes=[a8, a8], qstep=4, max_error=1, scalable_to=2)
    with pytest.raises(ValueError, match="frame 1: qstep has 3 steps, the frame has 4 channels"):
        geo.compress(pts, attributes=[a8, a84], qstep=(4, 4, 4), scalable_to=2)
    check = geo._check_scalable_to
    assert check(None, 0, 7, None, [a8], 0, False, None) == (None, None)
    assert check(None, 0, 1, [7, 7, 7], [a8], 0, False, None) == ([7, 7, 7], None)
    assert check(3, 0, 7, None, [a8, a84], 0, False, None) == ([7, 7, 7, 7], 3)      # an integer serves every channel
    assert check(np.int64(5), 10, 1, [1, 2, 3], [a8], 0, False, None) == ([1, 2, 3], 5)
