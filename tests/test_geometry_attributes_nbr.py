"""Attribute blob versions 25 and 26 on the host (include/pcc.h has the rule: lossless values predicted from up to three
Morton-first points of the coarser cells around a point): the numpy restatement tests/attr_nbr_ref.py against itself
and against the restatements of versions 1 and 2, one stream worked by hand, the decoder at a level of detail from the
cells alone, the size condition, the host-only entry points and the argument checks of compress(...,
predictor="neighbours").  No GPU."""
import os
import struct

import numpy as np
import pytest

import attr2_ref
import attr_cross_ref
import attr_nbr_ref as nbr
import attr_ref
from conftest import ROOT, pkg, random_cloud
from test_geometry_attributes_lod import RATE_MARGIN, _morton, _sample

MASKS = {1: (None,), 2: (None, True), 3: (None, True, (2,)), 4: (None, (1, 2), True)}


def _values(rng, pts, c, bpv):
    """smooth in space with noise, over the whole value range (so that residuals wrap)"""
    top = 1 << (8 * bpv)
    base = (pts.astype(np.int64) * np.array([3, 5, 7])).sum(1)[:, None] * (top // 256) + rng.integers(0, top)
    return ((base + rng.integers(0, 30 * (top // 256), (pts.shape[0], c))) % top).astype(np.int64)


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(2501)
    out = {n: _morton(random_cloud(rng, n, extent=40, lo=-20)[:, 1:], np.arange(n))[0] for n in (1, 2, 3, 65, 700)}
    out["origin"] = _morton(random_cloud(rng, 900, extent=24, lo=-12)[:, 1:], np.arange(900))[0]      # straddles 0 on every axis
    return out


@pytest.mark.parametrize("bpv", [1, 2])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_the_decoder_inverts_the_encoder(clouds, bpv, c):
    rng = np.random.default_rng(100 * bpv + c)
    for name, pts in clouds.items():
        vals = _values(rng, pts, c, bpv)
        plain = nbr.encode(pts, vals, bpv)
        for cross in MASKS[c]:
            blob = nbr.encode(pts[::-1], vals[::-1], bpv, cross=cross)          # any row order
            m = attr_cross_ref.mask_of(cross, c)
            assert blob[:4] == bytes([ord("A"), 26 if m else 25, bpv, c | (m << 4)]), (name, cross)
            assert struct.unpack_from("<II", blob, 4) == (pts.shape[0], len(blob) - 12)
            got, gb = nbr.decode(blob, pts)
            assert gb == bpv and np.array_equal(got, vals), (name, cross)
            assert m or blob == plain
    empty = nbr.encode(np.zeros((0, 3), np.int64), np.zeros((0, c), np.int64), bpv, cross=MASKS[c][-1])
    assert len(empty) == 12 and nbr.decode(empty, np.zeros((0, 3), np.int64))[0].shape == (0, c)


def test_the_layout_is_version_2s_under_another_version_byte(clouds):
    """the same cells[], S, chunks, p0 and words as a version-2 blob has of the same residuals: under version 2's head a
    version-25 blob is a well-formed version-2 blob, whose reader returns the residuals of the neighbour predictor"""
    rng = np.random.default_rng(7)
    pts = clouds[700]
    vals = _values(rng, pts, 3, 1)
    blob, v2 = nbr.encode(pts, vals, 1), attr2_ref.encode(pts, vals, 1)
    assert blob[12:12 + 72] == v2[12:12 + 72]                                # cells[16], S, n_chunks
    as2 = blob[:1] + bytes([2]) + blob[2:]
    keys, srt, order, s, idx, w = nbr.neighbours(pts)
    r, _ = attr2_ref._residuals(as2, 700)
    half = 128
    assert np.array_equal(r, (((vals - nbr.predict(vals, idx, w) + half) & 255) - half)[order])
    assert not np.array_equal(attr2_ref.decode(as2, pts)[0], vals)
    for bad in (1, 2, 11, 24, 27):
        with pytest.raises(AssertionError):
            nbr.decode(blob[:1] + bytes([bad]) + blob[2:], pts)


def test_hand_worked_stream():
    """Six points, one uint8 channel, small coordinates (the bias adds 0x8000 to each, which no xor or difference below
    sees).  Keys (x bit i at 3i + 2, y at 3i + 1, z at 3i) above 7 * 2^45:
        A (0,0,0) 0   B (0,0,1) 1   F (0,0,2) 8   E (0,2,0) 16   D (2,0,0) 32   G (4,0,0) 256      Morton order A B F E D G
    Sizes: A 16; B hb(1) = 0 -> 0; F hb(9) = 3 -> 1; E hb(24) = 4 -> 1; D hb(48) = 5 -> 1; G hb(288) = 8 -> 2.
    Introduction order: A, G, F, E, D, B.  cells = 6, 5, 2, 1, ..
    G (s 2): u = P >> 2 = (1,0,0), cells of side 8: only C = 0 holds points -> first(G) = A alone, d = 1; p = floor((2 *
      65536 * 100 + 65536) / (2 * 65536)) = 100.
    F (s 1): u = (0,0,1), cells of side 4: C = 0 -> A, d = 1; (1,0,0) -> G, G >> 1 = (2,0,0), d = 4 + 1 = 5, w = 13107.
      p = floor((2 (65536 * 100 + 13107 * 50) + 78643) / (2 * 78643)) = floor(14496543 / 157286) = 92.  E the same.
    D (s 1): u = (1,0,0): A d = 1, G d = 1: p = floor((2 * 65536 * 150 + 131072) / 262144) = floor(75.5) = 75.
    B (s 0): u = (0,0,1), cells of side 2: C = 0 -> A, d = 1; (0,0,1) -> F, d = 1; (0,1,0) -> E, d = 4 + 1 = 5;
      (1,0,0) -> D, d = 5.  Three candidates are kept: A and F (a tie at d = 1, both stay), and of the tie at d = 5 the
      smaller Morton index, E (3) before D (4).  p = floor((2 (65536 * 204 + 13107 * 96) + 144179) / (2 * 144179)) =
      floor(29399411 / 288358) = 101; with D in E's place it would be 104.
    Values A 100, B 90, F 104, E 96, D 120, G 50 -> residuals in introduction order 100, -50, 12, 4, 45, -11.
    At level 1 the cells are (0,0,0) {A, B}, (0,0,1) F, (0,1,0) E, (1,0,0) D, (2,0,0) G: five values 100, 104, 96, 120, 50
    from the first five residuals."""
    pts = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 2, 0], [2, 0, 0], [4, 0, 0]])
    vals = np.array([100, 90, 104, 96, 120, 50])
    keys, srt, order, s, idx, w = nbr.neighbours(pts)
    assert [int(k) - (7 << 45) for k in keys] == [0, 1, 8, 16, 32, 256] and list(srt) == list(range(6))
    assert list(s) == [16, 0, 1, 1, 1, 2] and list(order) == [0, 5, 2, 3, 4, 1]
    assert idx.tolist() == [[-1, -1, -1], [0, 2, 3], [0, 5, -1], [0, 5, -1], [0, 5, -1], [0, -1, -1]]
    assert w.tolist() == [[0, 0, 0], [65536, 65536, 13107], [65536, 13107, 0], [65536, 13107, 0], [65536, 65536, 0], [65536, 0, 0]]
    assert nbr.predict(vals[:, None], idx, w)[:, 0].tolist() == [0, 101, 92, 92, 75, 100]
    assert nbr.neighbours(pts, tie=-1)[4][1].tolist() == [2, 0, 4]           # the ties the other way: F before A, D for E
    blob = nbr.encode(pts, vals, 1)
    assert blob[:12] == bytes([ord("A"), 25, 1, 1]) + struct.pack("<II", 6, len(blob) - 12)
    assert struct.unpack_from("<16I", blob, 12) == (6, 5, 2) + (1,) * 13 and struct.unpack_from("<II", blob, 76) == (1, 1)
    assert nbr.residuals(blob, 6)[0][:, 0].tolist() == [100, -50, 12, 4, 45, -11]
    assert nbr.decode(blob, pts)[0][:, 0].tolist() == vals.tolist()
    nbytes, m = nbr.lod_info(blob, 1)
    assert m == 5 and nbytes <= len(blob)                                    # S = 1: lane 5 alone is cut, and its run may be empty
    cells = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [2, 0, 0]])
    assert nbr.decode(blob[:nbytes], cells, 1)[0][:, 0].tolist() == [100, 104, 96, 120, 50]
    assert nbr.encode(pts, vals, 1, tie=-1) != blob


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_the_decoder_at_a_level_sees_only_the_cells(clouds, k):
    """from the shortest prefix and the cells points >> k: the value of the Morton-first point of every cell, as version
    2 defines a level; also for a sender's side level (slod) and for a frame around the origin"""
    rng = np.random.default_rng(31 + k)
    for name in (700, "origin", 3):
        pts = clouds[name]
        for c, bpv, cross in ((1, 1, None), (3, 2, None), (4, 1, (1, 2))):
            vals = _values(rng, pts, c, bpv)
            blob = nbr.encode(pts, vals, bpv, cross=cross)
            wc, wv = _sample(pts, vals, k)
            nbytes, m = nbr.lod_info(blob, k)
            assert m == wc.shape[0] and (nbytes == len(blob) if k == 0 else nbytes <= len(blob))
            got, _ = nbr.decode(blob[:nbytes], wc[::-1], k)                    # any row order
            assert np.array_equal(got, wv), (name, c, k)
            if nbytes > 400:
                with pytest.raises(AssertionError):
                    nbr.decode(blob[:nbytes - 2], wc, k)
    # a sender at level 2: the blob of the cells under the bias 32768 >> 2, cut again by a receiver at k
    pts = clouds["origin"]
    u = np.unique(pts >> 2, axis=0)
    u = u[np.argsort(attr2_ref.keys_of(u, 32768 >> 2))]
    vals = _values(rng, u, 2, 1)
    blob = nbr.encode(u, vals, 1, bias=32768 >> 2)
    assert blob[2] == 1 | (2 << 4)
    _, first = np.unique(attr2_ref.keys_of(u >> k, 32768 >> (2 + k)), return_index=True)
    nbytes, m = nbr.lod_info(blob, k)
    assert m == first.shape[0]
    assert np.array_equal(nbr.decode(blob[:nbytes], u[first] >> k, k)[0], vals[first])


def test_lod_info_is_version_2s_formula(clouds):
    """the residuals differ, the layout does not: (bytes, values) follow from cells[], S and the chunks' length tables
    exactly as attr_blob.h states for version 2, and the library's host entry points agree"""
    G = pkg().GeometryCodec
    rng = np.random.default_rng(5)
    pts = _morton(random_cloud(rng, 9000, extent=60, lo=-30)[:, 1:], np.arange(9000))[0]      # c = 4: S = 128, two chunks
    for c, cross in ((1, None), (4, None), (4, (1, 3))):
        vals = _values(rng, pts, c, 1)
        blob = nbr.encode(pts, vals, 1, cross=cross)
        off = 12 + 72
        cells = struct.unpack_from("<16I", blob, 12)
        S, nc = struct.unpack_from("<II", blob, 76)
        words = struct.unpack_from("<%dI" % nc, blob, off + 2 * attr_ref.contexts(1, c))
        payload = off + 2 * attr_ref.contexts(1, c) + 4 * nc
        for k in range(16):
            if k == 0:
                want = (len(blob), 9000)
            else:
                lanes = -(-cells[k] // S)
                cs, ls = (lanes - 1) // 64, (lanes - 1) % 64
                start = payload + 2 * sum(words[:cs])
                lens = np.frombuffer(blob, "<u2", 64, start + 256)
                want = (start + 2 * (192 + int(lens[:ls + 1].sum())), cells[k])
            assert nbr.lod_info(blob, k) == want, (c, k)
            assert G.attr_lod_info(blob, k) == want, (c, k)
            assert G.attr_lod_info(blob[:want[0]], k) == want, (c, k)
        info = G.attr_info(blob)
        assert info["version"] == (26 if cross else 25) and info["scalable"] and info["predictor"] == "neighbours" and info["max_error"] == 0
        assert info.get("cross_channel") == cross and info["points"] == 9000 and info["channels"] == c
    assert "predictor" not in G.attr_info(attr2_ref.encode(pts, vals, 1))


def test_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    assert "pcc_attr_encode_frames_nbr(" in text and "pcc_attr_encode_frames_nbr" in abi.PROTOTYPES
    assert hasattr(abi.lib(), "pcc_attr_encode_frames_nbr")


def _zed(i):
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        u, mean = attr_ref.merge(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"])
    return _morton(u, mean)


def _sizes(pts, vals):
    v1, v2, v25 = len(attr_ref.encode(vals, 1)), len(attr2_ref.encode(pts, vals, 1)), len(nbr.encode(pts, vals, 1))
    print(f"version 1 {v1} B, version 2 {v2} B, version 25 {v25} B: {v25 / v2 - 1:+.4f} against 2, {v25 / v1 - 1:+.4f} against 1, "
          f"{8 * v25 / vals.size:.3f} bits per value")
    return v1, v2, v25


def test_rate_on_recorded_colour():
    """ZED frame 0 RGB (19 679 points): version 1 42606 B, version 2 42068 B, version 25 38754 B (-7.9 % / -9.0 %)"""
    v1, v2, v25 = _sizes(*_zed(0))
    assert v25 < v2 and v25 < v1


def test_rate_on_room_colour(wl):
    """workloads.room(200000) RGB: version 1 439126 B, version 2 434990 B, version 25 393814 B (-9.5 % / -10.3 %)"""
    room = wl.room(200_000, seed=0)
    v1, v2, v25 = _sizes(*_morton(room["points"], np.rint(255 * room["colors"]).astype(np.int64)))
    assert v25 < v2 and v25 < v1


def test_rate_on_sweep_intensity(wl):
    """the sweep of test_rate_against_version_1 (lidar_sweep(seed=1), lidar_intensity(seed=1)): version 25 stays within the
    allowance that test grants version 2 over version 1"""
    sweep = wl.lidar_sweep(seed=1)["points"]
    v1, v2, v25 = _sizes(*_morton(sweep, wl.lidar_intensity(sweep, seed=1).astype(np.int64)[:, None]))
    assert v25 <= (1 + RATE_MARGIN[0]) * v1


def test_compress_checks_the_predictor():
    """the checks of compress that run before the runtime is entered: on an instance that has none"""
    G = pkg().GeometryCodec
    geo = object.__new__(G)
    pts = [np.zeros((3, 3), np.int32) + np.arange(3, dtype=np.int32)[:, None]] * 2
    a8 = np.zeros((3, 3), np.uint8)
    for bad in (True, 1, 2.0, ("neighbours",), b"neighbours"):
        with pytest.raises(TypeError, match="predictor must be None or 'neighbours'"):
            geo.compress(pts, attributes=[a8, a8], predictor=bad)
    for bad in ("neighbors", "", "first", "Neighbours"):
        with pytest.raises(ValueError, match="predictor must be None or 'neighbours'"):
            geo.compress(pts, attributes=[a8, a8], predictor=bad)
    with pytest.raises(ValueError, match="it needs attributes="):
        geo.compress(pts, predictor="neighbours")
    for kw in (dict(max_error=1), dict(qstep=4), dict(qstep=(4, 4, 4)), dict(qstep=4, colour="ycocg"), dict(colour="ycocg"),
               dict(qstep=4, scalable_to=2), dict(scalable_to=2), dict(qstep=4, target_bytes=100), dict(target_bytes=[100, 100]),
               dict(qstep=4, target_frame_bytes=100)):
        name = next(n for n in ("max_error", "qstep", "colour", "scalable_to", "target_bytes", "target_frame_bytes") if n in kw)
        with pytest.raises(ValueError, match=f"predictor='neighbours' with {name}: attribute blob versions 25 and 26 are lossless"):
            geo.compress(pts, attributes=[a8, a8], predictor="neighbours", **kw)
    with pytest.raises(ValueError, match="cross_channel names channel 3"):
        geo.compress(pts, attributes=[a8, a8], predictor="neighbours", cross_channel=(3,))
    # the record of the one encode binding: version 2's family, and what contradicts it
    AttrCoding = pkg("runtime").AttrCoding
    assert AttrCoding.of(2, neighbours=True).entry(False) == "_nbr" and AttrCoding.of(2, neighbours=True).entry(True) == "_nbr"
    assert AttrCoding.of(2, cross=[3, 0], neighbours=True).entry(False) == "_nbr"
    for kw in (dict(max_error=2), dict(qstep=4), dict(qstep=4, scalable_to=2)):
        with pytest.raises(ValueError):
            AttrCoding.of(2, neighbours=True, **kw)
