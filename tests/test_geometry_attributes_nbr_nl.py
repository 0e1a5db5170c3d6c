"""Attribute blob versions 28 and 31 on the host (include/pcc.h has the rule: the bounded-error forms of versions 25 and
26, a closed loop over the decoded values of up to three candidates): the numpy restatement tests/attr_nbr_nl_ref.py
against itself and against the lossless restatement, one stream worked by hand, the decoder at a level of detail from
the cells alone, the host-only entry points, the argument checks of compress(..., predictor="bounded-neighbours") and
the rates against versions 7 and 14 with the reference coders.  No GPU."""
import os
import struct

import numpy as np
import pytest

import attr2_ref
import attr_cross_ref
import attr_nbr_nl_ref as nnl
import attr_nbr_ref as nbr
import attr_nl_ref
import attr_ref
from conftest import ROOT, pkg, random_cloud
from test_geometry_attributes_lod import _morton, _sample

MASKS = {1: (None,), 2: (None, True), 3: (None, True, (2,)), 4: (None, (1, 2), True)}
ERRORS = {1: (1, 2, 127), 2: (1, 2, 32767)}


def _values(rng, pts, c, bpv):
    """smooth in space with noise, over the whole value range, with values at both ends of it"""
    top = 1 << (8 * bpv)
    base = (pts.astype(np.int64) * np.array([3, 5, 7])).sum(1)[:, None] * (top // 256) + rng.integers(0, top)
    v = ((base + rng.integers(0, 30 * (top // 256), (pts.shape[0], c))) % top).astype(np.int64)
    v[rng.random(v.shape) < 0.02] = 0
    v[rng.random(v.shape) < 0.02] = top - 1
    return v


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(2831)
    out = {n: _morton(random_cloud(rng, n, extent=40, lo=-20)[:, 1:], np.arange(n))[0] for n in (1, 2, 700)}
    out["origin"] = _morton(random_cloud(rng, 900, extent=24, lo=-12)[:, 1:], np.arange(900))[0]      # straddles 0 on every axis
    out[9000] = _morton(random_cloud(rng, 9000, extent=60, lo=-30)[:, 1:], np.arange(9000))[0]
    return out


@pytest.mark.parametrize("bpv", [1, 2])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_the_decoder_inverts_the_encoder_within_e(clouds, bpv, c):
    rng = np.random.default_rng(100 * bpv + c)
    mask = (1 << (8 * bpv)) - 1
    for name in (1, 2, 700, 9000):
        pts = clouds[name]
        vals = _values(rng, pts, c, bpv)
        for e in (ERRORS[bpv] if name != 9000 else ERRORS[bpv][c % 3:][:1]):      # the large cloud: one e and one mask per (bpv, c)
            plain = nnl.encode(pts, vals, bpv, e)
            for cross in (MASKS[c] if name != 9000 else MASKS[c][-1:]):
                blob = nnl.encode(pts[::-1], vals[::-1], bpv, e, cross=cross)      # any row order
                m = attr_cross_ref.mask_of(cross, c)
                assert blob[:4] == bytes([ord("A"), 31 if m else 28, bpv, c | (m << 4)]), (name, cross)
                assert struct.unpack_from("<III", blob, 4) == (pts.shape[0], len(blob) - 12, e)
                got, gb = nnl.decode(blob, pts)
                assert gb == bpv and got.min() >= 0 and got.max() <= mask and np.abs(got - vals).max() <= e, (name, cross, e)
                assert np.array_equal(got, nnl.decode(plain, pts)[0]), "the cross form decodes to the plain form's values"
                assert m or blob == plain
    for e in ERRORS[bpv]:
        empty = nnl.encode(np.zeros((0, 3), np.int64), np.zeros((0, c), np.int64), bpv, e, cross=MASKS[c][-1])
        assert len(empty) == 12 and empty[1] == (31 if c > 1 else 28)
        assert nnl.decode(empty, np.zeros((0, 3), np.int64))[0].shape == (0, c)


def test_the_layout_is_version_7s_under_another_version_byte(clouds):
    """max_error, cells[], S, n_chunks as a version-7 blob of the same points has them; under version 7's head the blob
    is a well-formed version-7 blob whose reader returns the closed loop's indices, and whose own decoder (sums along
    the chains of first()) returns other values"""
    rng = np.random.default_rng(7)
    pts = clouds[700]
    vals = _values(rng, pts, 3, 1)
    blob, v7 = nnl.encode(pts, vals, 1, 2), attr_nl_ref.encode(vals, 1, 2, points=pts)
    assert blob[12:12 + 76] == v7[12:12 + 76]                                # max_error, cells[16], S, n_chunks
    as7 = blob[:1] + bytes([7]) + blob[2:]
    keys, srt, order, s, idx, w = nbr.neighbours(pts)
    j, vh = nnl.closed_loop(vals, s, idx, w, 2, 255)
    b2, e = attr_nl_ref._lossless_shape(as7)
    assert e == 2 and np.array_equal(attr2_ref._residuals(b2, 700)[0], j[order])
    assert np.array_equal(nnl.decode(blob, pts)[0], vh)
    for bad in (2, 7, 14, 25, 26, 29, 30):
        with pytest.raises(AssertionError):
            nnl.decode(blob[:1] + bytes([bad]) + blob[2:], pts)


def test_hand_worked_stream():
    """The six points of version 25's hand-worked stream, one uint8 channel, e = 5, q = 11.  Morton order A B F E D G,
    sizes 16, 0, 1, 1, 1, 2, introduction order A, G, F, E, D, B, candidates and weights as worked there: G <- A;
    F, E <- A (w 65536), G (w 13107); D <- A, G (65536 each); B <- A, F (a tie at d = 1, both stay) and, of the tie at
    d = 5, E (Morton index 3) before D (4), w 13107.
    Values A 255, B 252, F 3, E 100, D 254, G 40.
    A: p = 0, d = 255, j = floor(260 / 11) = 23, v^ = 253.
    G: p = floor((2 * 65536 * 253 + 65536) / 131072) = 253, d = -213, j = -floor(218 / 11) = -19, v^ = 253 - 209 = 44.
    F: p = floor((2 (65536 * 253 + 13107 * 44) + 78643) / 157286) = floor(34393275 / 157286) = 218, d = -215,
       j = -floor(220 / 11) = -20, p + j q = -2: clamped to 0 (|3 - 0| <= 5).
    E: p = 218, d = -118, j = -floor(123 / 11) = -11, v^ = 218 - 121 = 97.
    D: p = floor((2 * 65536 * (253 + 44) + 131072) / 262144) = 149, d = 105, j = floor(110 / 11) = 10, p + j q = 259:
       clamped to 255.
    B: over the DECODED values 253, 0, 97: p = floor((2 (65536 * 253 + 65536 * 0 + 13107 * 97) + 144179) / 288358) =
       floor(35848153 / 288358) = 124, d = 128, j = floor(133 / 11) = 12, p + j q = 256: clamped to 255.  With D in E's
       place p would be 138, over the merged values 255, 3, 100 instead of the decoded ones 126.
    Indices in introduction order 23, -19, -20, -11, 10, 12; decoded values 253, 255, 0, 97, 255, 44.
    At level 1 the cells are (0,0,0) {A, B}, (0,0,1) F, (0,1,0) E, (1,0,0) D, (2,0,0) G: 253, 0, 97, 255, 44 from the
    first five indices."""
    pts = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 2, 0], [2, 0, 0], [4, 0, 0]])
    vals = np.array([255, 252, 3, 100, 254, 40])
    keys, srt, order, s, idx, w = nbr.neighbours(pts)
    assert list(order) == [0, 5, 2, 3, 4, 1] and idx[1].tolist() == [0, 2, 3] and w[1].tolist() == [65536, 65536, 13107]
    j, vh = nnl.closed_loop(vals[:, None], s, idx, w, 5, 255)
    assert j[order, 0].tolist() == [23, -19, -20, -11, 10, 12]
    assert vh[:, 0].tolist() == [253, 255, 0, 97, 255, 44]
    assert nbr.predict(vh, idx, w)[:, 0].tolist() == [0, 124, 218, 218, 149, 253]
    assert nbr.predict(vals[:, None], idx, w)[1, 0] == 126
    blob = nnl.encode(pts, vals, 1, 5)
    assert blob[:16] == bytes([ord("A"), 28, 1, 1]) + struct.pack("<III", 6, len(blob) - 12, 5)
    assert struct.unpack_from("<16I", blob, 16) == (6, 5, 2) + (1,) * 13 and struct.unpack_from("<II", blob, 80) == (1, 1)
    assert nnl.decode(blob, pts)[0][:, 0].tolist() == [253, 255, 0, 97, 255, 44]
    assert np.abs(nnl.decode(blob, pts)[0][:, 0] - vals).max() == 4
    nbytes, m = nnl.lod_info(blob, 1)
    assert m == 5 and nbytes <= len(blob)
    cells = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [2, 0, 0]])
    assert nnl.decode(blob[:nbytes], cells, 1)[0][:, 0].tolist() == [253, 0, 97, 255, 44]


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_the_decoder_at_a_level_sees_only_the_cells(clouds, k):
    """from the shortest prefix and the cells points >> k: v^ of the Morton-first point of every cell, which is the row
    of the whole decode and lies within e of the lossless kinds' row at that lod; also for a sender's side level"""
    rng = np.random.default_rng(31 + k)
    for name in (700, "origin", 2):
        pts = clouds[name]
        for c, bpv, e, cross in ((1, 1, 1, None), (3, 2, 300, None), (4, 1, 2, (1, 2))):
            vals = _values(rng, pts, c, bpv)
            blob = nnl.encode(pts, vals, bpv, e, cross=cross)
            whole = nnl.decode(blob, pts)[0]
            wc, wv = _sample(pts, vals, k)
            nbytes, m = nnl.lod_info(blob, k)
            assert m == wc.shape[0] and (nbytes == len(blob) if k == 0 else nbytes <= len(blob))
            got, _ = nnl.decode(blob[:nbytes], wc[::-1], k)                    # any row order
            assert np.array_equal(got, _sample(pts, whole, k)[1]), (name, c, k)
            lb = nbr.encode(pts, vals, bpv, cross=cross)
            lossless = nbr.decode(lb[:nbr.lod_info(lb, k)[0]], wc, k)[0]
            assert np.array_equal(lossless, wv) and np.abs(got - lossless).max() <= e, (name, c, k)
            if nbytes > 400:
                with pytest.raises(AssertionError):
                    nnl.decode(blob[:nbytes - 2], wc, k)
    # a sender at level 2 (a bias below 32768): the blob of the cells under 32768 >> 2, cut again by a receiver at k
    pts = clouds["origin"]
    u = np.unique(pts >> 2, axis=0)
    u = u[np.argsort(attr2_ref.keys_of(u, 32768 >> 2))]
    vals = _values(rng, u, 2, 1)
    blob = nnl.encode(u, vals, 1, 2, bias=32768 >> 2)
    assert blob[2] == 1 | (2 << 4)
    whole = nnl.decode(blob, u)[0]
    _, first = np.unique(attr2_ref.keys_of(u >> k, 32768 >> (2 + k)), return_index=True)
    nbytes, m = nnl.lod_info(blob, k)
    assert m == first.shape[0]
    got = nnl.decode(blob[:nbytes], u[first] >> k, k)[0]
    assert np.array_equal(got, whole[first]) and np.abs(got - vals[first]).max() <= 2


def test_lod_info_is_version_7s_formula_and_attr_info(clouds):
    """(bytes, values) follow from cells[], S and the chunks' length tables exactly as for version 7 (the four bytes of
    max_error in front), and the library's host entry points agree with the reference on its blobs"""
    G = pkg().GeometryCodec
    rng = np.random.default_rng(5)
    pts = clouds[9000]                                                       # c = 4: S = 128, two chunks
    for c, e, cross in ((1, 1, None), (4, 2, None), (4, 127, (1, 3))):
        vals = _values(rng, pts, c, 1)
        blob = nnl.encode(pts, vals, 1, e, cross=cross)
        off = 12 + 4 + 72
        cells = struct.unpack_from("<16I", blob, 16)
        S, nc = struct.unpack_from("<II", blob, 80)
        words = struct.unpack_from("<%dI" % nc, blob, off + 2 * attr_ref.contexts(1, c))
        payload = off + 2 * attr_ref.contexts(1, c) + 4 * nc
        as7 = blob[:1] + bytes([14 if cross else 7]) + blob[2:]
        for k in range(16):
            if k == 0:
                want = (len(blob), 9000)
            else:
                lanes = -(-cells[k] // S)
                cs, ls = (lanes - 1) // 64, (lanes - 1) % 64
                start = payload + 2 * sum(words[:cs])
                lens = np.frombuffer(blob, "<u2", 64, start + 256)
                want = (start + 2 * (192 + int(lens[:ls + 1].sum())), cells[k])
            assert nnl.lod_info(blob, k) == want, (c, k)
            assert G.attr_lod_info(blob, k) == want == G.attr_lod_info(as7, k), (c, k)
            assert G.attr_lod_info(blob[:want[0]], k) == want, (c, k)
        info = G.attr_info(blob)
        assert info["version"] == (31 if cross else 28) and info["scalable"] is True and info["predictor"] == "neighbours"
        assert info["max_error"] == e and info.get("cross_channel") == cross and info["points"] == 9000 and info["channels"] == c
        assert info["lod"] == 0 and info["bpv"] == 1
        ref = nnl.info(blob)
        assert all(info[key] == ref[key] for key in ("version", "bpv", "channels", "points", "max_error", "scalable", "lod", "predictor"))
    assert G.attr_info(attr_nl_ref.encode(vals, 1, 2, points=pts)).get("predictor") is None
    assert G.attr_info(nbr.encode(pts, vals, 1))["max_error"] == 0
    empty = nnl.encode(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), 2, 9, cross=True)
    info = G.attr_info(empty)
    assert info["version"] == 31 and info["points"] == 0 and info["cross_channel"] == (1, 2) and info["predictor"] == "neighbours"
    # a head that lies about its bound: 0, and 2^(8 bpv - 1)
    Err = pkg("_abi").PccError
    for bad in (0, 128):
        with pytest.raises(Err):
            G.attr_info(blob[:12] + struct.pack("<I", bad) + blob[16:])
        with pytest.raises(Err):
            G.attr_lod_info(blob[:12] + struct.pack("<I", bad) + blob[16:], 1)


def test_compress_checks_the_bounded_predictor():
    """the checks of compress that run before the runtime is entered: on an instance that has none"""
    G = pkg().GeometryCodec
    geo = object.__new__(G)
    pts = [np.zeros((3, 3), np.int32) + np.arange(3, dtype=np.int32)[:, None]] * 2
    a8, a16 = np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.uint16)
    for kw in (dict(), dict(max_error=0)):
        with pytest.raises(ValueError, match="'neighbours' is the lossless kind"):
            geo.compress(pts, attributes=[a8, a8], predictor="bounded-neighbours", **kw)
    with pytest.raises(ValueError, match="it needs attributes="):
        geo.compress(pts, predictor="bounded-neighbours", max_error=2)
    for kw in (dict(qstep=4), dict(qstep=(4, 4, 4)), dict(qstep=4, colour="ycocg"), dict(colour="ycocg"),
               dict(qstep=4, scalable_to=2), dict(scalable_to=2), dict(qstep=4, target_bytes=100), dict(target_bytes=[100, 100]),
               dict(qstep=4, target_frame_bytes=100)):
        name = next(n for n in ("qstep", "colour", "scalable_to", "target_bytes", "target_frame_bytes") if n in kw)
        with pytest.raises(ValueError, match=f"predictor='bounded-neighbours' with {name}"):
            geo.compress(pts, attributes=[a8, a8], predictor="bounded-neighbours", max_error=2, **kw)
    # max_error's own checks are the ones of before
    for bad in (True, 1.0, "2"):
        with pytest.raises(TypeError, match="max_error must be an integer >= 0"):
            geo.compress(pts, attributes=[a8, a8], predictor="bounded-neighbours", max_error=bad)
    with pytest.raises(ValueError, match="max_error must be an integer >= 0"):
        geo.compress(pts, attributes=[a8, a8], predictor="bounded-neighbours", max_error=-1)
    with pytest.raises(ValueError, match="frame 1: max_error 128 is too large for uint8"):
        geo.compress(pts, attributes=[a16, a8], predictor="bounded-neighbours", max_error=128)
    with pytest.raises(ValueError, match="max_error 32768 is too large for uint16"):
        geo.compress(pts, attributes=[a16, a16], predictor="bounded-neighbours", max_error=32768)
    with pytest.raises(ValueError, match="cross_channel names channel 3"):
        geo.compress(pts, attributes=[a8, a8], predictor="bounded-neighbours", max_error=1, cross_channel=(3,))
    # the lossless spelling keeps refusing max_error, and now says where the bounded form is
    with pytest.raises(ValueError, match="predictor='neighbours' with max_error: attribute blob versions 25 and 26 are lossless.*'bounded-neighbours'"):
        geo.compress(pts, attributes=[a8, a8], predictor="neighbours", max_error=1)
    for bad in ("bounded", "bounded-neighbors", "near-lossless"):
        with pytest.raises(ValueError, match="predictor must be None or 'neighbours'"):
            geo.compress(pts, attributes=[a8, a8], predictor=bad, max_error=1)
    # the record of the one encode binding
    AttrCoding = pkg("runtime").AttrCoding
    rec = AttrCoding.of(2, max_error=2, neighbours_nl=True)
    assert rec.entry(False) == "_nbr_nl" and rec.entry(True) == "_nbr_nl" and rec.max_error == 2 and not rec.neighbours
    assert AttrCoding.of(2, max_error=1, cross=[3, 0], neighbours_nl=True).entry(False) == "_nbr_nl"
    for kw in (dict(), dict(max_error=0), dict(max_error=2, qstep=4), dict(max_error=2, neighbours=True), dict(max_error=2, targets=[9])):
        with pytest.raises(ValueError):
            AttrCoding.of(2, neighbours_nl=True, **kw)
    with pytest.raises(ValueError):
        AttrCoding.of(2, neighbours=True, max_error=2)


def test_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    assert "pcc_attr_encode_frames_nbr_nl(" in text and "pcc_attr_encode_frames_nbr_nl" in abi.PROTOTYPES
    assert hasattr(abi.lib(), "pcc_attr_encode_frames_nbr_nl")
    assert len(abi.PROTOTYPES["pcc_attr_encode_frames_nbr_nl"][1]) == len(abi.PROTOTYPES["pcc_attr_encode_frames_nbr"][1]) + 1


# ---- rates with the reference coders, at e = 2, on the inputs the feature was priced on ------------------------------
E = 2


def _zed(i):
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        u, mean = attr_ref.merge(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"])
    return _morton(u, mean)


def _v14(pts, vals, e):
    """version 14's bytes with the reference coders: version 7's indices under the cross rule"""
    keys = attr2_ref.keys_of(pts, 32768)
    s, order, first = attr2_ref.intro(keys)
    j, _ = attr_nl_ref.indices7(vals.astype(np.int64), s, first, e)
    m = attr_cross_ref.mask_of(True, vals.shape[1])
    return 12 + 4 + 64 + len(attr_nl_ref._code(attr_cross_ref.forward(j[order], m, 1), 1))


def _sizes(pts, vals, cross=False):
    v7, new = len(attr_nl_ref.encode(vals, 1, E, points=pts)), len(nnl.encode(pts, vals, 1, E))
    print(f"e = {E}: version 7 {v7} B, version 28 {new} B ({new / v7 - 1:+.4f})")
    if not cross:
        return v7, new
    v14, newx = _v14(pts, vals, E), len(nnl.encode(pts, vals, 1, E, cross=True))
    print(f"e = {E}: version 14 {v14} B, version 31 {newx} B ({newx / v14 - 1:+.4f})")
    return v7, new, v14, newx


def test_rate_on_recorded_colour():
    """ZED frame 0 RGB (19 679 points), e = 2: version 7 25624 B, version 28 22148 B (-13.6 %); version 14 20440 B,
    version 31 17354 B (-15.1 %)"""
    v7, new, v14, newx = _sizes(*_zed(0), cross=True)
    assert new < v7 and newx < v14


def test_rate_on_room_colour(wl):
    """workloads.room(60000, seed=0) RGB, e = 2: version 7 90092 B, version 28 77114 B (-14.4 %)"""
    room = wl.room(60000, seed=0)
    v7, new = _sizes(*_morton(room["points"], np.rint(255 * room["colors"]).astype(np.int64)))
    assert new < v7


def test_rate_on_sweep_intensity(wl):
    """lidar_sweep(seed=1) with lidar_intensity(seed=1), e = 2: version 7 23604 B, version 28 21832 B (-7.5 %)"""
    sweep = wl.lidar_sweep(seed=1)["points"]
    v7, new = _sizes(*_morton(sweep, wl.lidar_intensity(sweep, seed=1).astype(np.int64)[:, None]))
    assert new <= v7
