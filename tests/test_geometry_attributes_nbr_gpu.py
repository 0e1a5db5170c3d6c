"""Attribute blob versions 25 and 26 on the GPU (compress(..., attributes=..., predictor="neighbours"); include/pcc.h has
the rule): every encode is compared byte for byte against the numpy restatement tests/attr_nbr_ref.py, every decode
against the merged input values, and at a level of detail against the value of the Morton-first point of every cell.
Frames stay at a few thousand points."""
import struct

import numpy as np
import pytest

import attr2_ref
import attr_nbr_ref as nbr
import attr_ref
from conftest import pkg, random_cloud
from test_geometry_attributes_lod import _sample


@pytest.fixture(scope="module")
def geo():
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _ref(p, a, k=0, cross=None):
    """the cells p >> k in Morton order, their merged values, and the restatement's blob of them"""
    a2 = a if a.ndim == 2 else a[:, None]
    u, mean = attr_ref.merge(np.asarray(p, np.int32).reshape(-1, 3) >> k, a2)
    o = np.argsort(attr2_ref.keys_of(u, 32768 >> k))
    return u[o], mean[o], nbr.encode(u, mean, a.dtype.itemsize, bias=32768 >> k, cross=cross)


def _check(geo, frames, attrs, cross_channel=False, masks=None, lod=0):
    """compress under the keyword: the blobs are the restatement's, and decode to the merged values"""
    gb, ab = geo.compress(frames, attributes=attrs, predictor="neighbours", cross_channel=cross_channel, lod=lod)
    assert gb == geo.compress(frames, lod=lod)
    cells, vals = geo.decompress(gb, ab)
    for f, (p, a) in enumerate(zip(frames, attrs)):
        u, mean, want = _ref(p, a, lod, None if masks is None else masks[f])
        assert ab[f] == want, f"frame {f}: {len(ab[f])} bytes, the restatement {len(want)}; head {ab[f][:12].hex()} / {want[:12].hex()}"
        assert np.array_equal(cells[f], u) and vals[f].dtype == a.dtype and np.array_equal(vals[f], mean), f
    return gb, ab


def _colour(rng, pts, c, dtype):
    """smooth in space, so that a predictor has something to find, with noise"""
    top = np.iinfo(dtype).max
    base = (pts.astype(np.int64) * np.array([3, 5, 7])).sum(1)[:, None] * (top // 255) + rng.integers(0, 40 * (top // 255), (pts.shape[0], c))
    return (base % (top + 1)).astype(dtype)


@pytest.mark.gpu
def test_one_two_three_points_an_empty_frame_and_one_past_a_block(geo):
    rng = np.random.default_rng(251)
    frames = [random_cloud(rng, n, extent=40, lo=-20)[:, 1:].astype(np.int32) if n else np.zeros((0, 3), np.int32) for n in (1, 2, 3, 0, 257)]
    attrs = [_colour(rng, p, 3, np.uint8) for p in frames]
    gb, ab = _check(geo, frames, attrs)
    assert [b[1] for b in ab] == [25] * 5 and len(ab[3]) == 12
    G = pkg().GeometryCodec
    assert G.attr_info(ab[4]) == {"version": 25, "bpv": 1, "channels": 3, "points": 257, "max_error": 0, "scalable": True, "lod": 0,
                                  "predictor": "neighbours"}
    assert G.attr_info(ab[3])["predictor"] == "neighbours" and G.attr_info(ab[3])["points"] == 0


@pytest.mark.gpu
def test_points_on_a_straight_line(geo):
    """only 3 of the 27 cells around a point can hold one: o = (-1, 0, 0), 0 and (1, 0, 0).  A point of size s sits in
    the upper half of its cell C (u = 2 C + 1), so first(C) and first(C + 1) are at d = 1 and first(C - 1) at d = 9:
    three candidates where the line goes on to both sides, and a tie in d between the first two"""
    rng = np.random.default_rng(252)
    line = np.stack([np.arange(-150, 150), np.full(300, 7), np.full(300, -3)], 1).astype(np.int32)
    diag = np.stack([np.arange(-100, 100)] * 3, 1).astype(np.int32)
    keys, srt, order, s, idx, w = nbr.neighbours(line)
    have = idx >= 0
    assert have.sum(1).max() == 3 and (w[:, 0][have[:, 0]] == 65536).all()
    assert set(w[have[:, 2], 2].tolist()) <= {65536 // 9, 65536 // 4}       # d = 4 where the line begins inside the cell C - 1
    frames = [line, diag]
    _check(geo, frames, [_colour(rng, p, 2, np.uint8) for p in frames])


@pytest.mark.gpu
def test_dense_block_where_the_morton_index_breaks_ties(geo):
    """16^3 points: all 27 cells occupied around the inner points and several candidates at one distance; the reference
    with the tie-break reversed gives other bytes, so the frame really contains ties that decide"""
    rng = np.random.default_rng(253)
    g = np.arange(16)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32) + np.array([-5, 20, 3], np.int32)
    vals = rng.integers(0, 256, (block.shape[0], 3)).astype(np.uint8)
    u, mean, want = _ref(block, vals)
    assert nbr.encode(u, mean, 1, tie=-1) != want
    assert not np.array_equal(nbr.decode(want, u, tie=-1)[0], mean)
    _check(geo, [block], [vals])


@pytest.mark.gpu
def test_points_at_the_lattice_edges(geo):
    """coordinates -32768 and 32767: candidate cells beyond the lattice are skipped, on both sides of every axis"""
    rng = np.random.default_rng(254)
    corners = np.array([[x, y, z] for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)], np.int32)
    near = np.concatenate([np.array([-32768, -32768, -32768]) + random_cloud(rng, 400, extent=24, lo=0)[:, 1:],
                           np.array([32767, 32767, 32767]) - random_cloud(rng, 400, extent=24, lo=0)[:, 1:],
                           np.array([32767, -32768, 0]) + random_cloud(rng, 300, extent=20, lo=0)[:, 1:] * np.array([-1, 1, 1])])
    pts = np.unique(np.concatenate([corners, near]).astype(np.int32), axis=0)
    assert pts.min() == -32768 and pts.max() == 32767
    _check(geo, [pts], [_colour(rng, pts, 3, np.uint8)])


@pytest.mark.gpu
def test_frame_that_straddles_the_origin(geo):
    """points on both sides of 0 on every axis differ in the top bit of the biased coordinates: sizes up to 15"""
    rng = np.random.default_rng(255)
    pts = random_cloud(rng, 3000, extent=60, lo=-30)[:, 1:].astype(np.int32)
    assert (pts.min(0) < 0).all() and (pts.max(0) > 0).all()
    assert nbr.neighbours(pts)[3][1:].max() == 15
    _check(geo, [pts], [_colour(rng, pts, 1, np.uint16)[:, 0]])


@pytest.mark.gpu
def test_sender_side_lod_2(geo):
    """compress(..., lod=2): the cells' means over the cells' keys, the lattice 65536 >> 2, slod in the head"""
    rng = np.random.default_rng(256)
    pts = random_cloud(rng, 4000, extent=80, lo=-40)[:, 1:].astype(np.int32)
    edge = np.array([[-32768, -32768, -32768], [32767, 32767, 32767], [32764, -32765, 5]], np.int32)
    frames = [pts, np.concatenate([pts[:500], edge])]
    gb, ab = _check(geo, frames, [_colour(rng, p, 3, np.uint8) for p in frames], lod=2)
    assert all(b[1] == 25 and b[2] >> 4 == 2 for b in ab)
    assert pkg().GeometryCodec.attr_info(ab[0])["lod"] == 2


@pytest.mark.gpu
def test_uint16_extremes_alternating_among_neighbours(geo):
    """0 and 65535 in a checkerboard: weighted sums of three 65535 x 65536 (beyond 32 bits) and residuals that wrap"""
    g = np.arange(12)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int32) - 6
    vals = np.where(block.sum(1) % 2 == 0, 0, 65535).astype(np.uint16)
    two = np.stack([vals, 65535 - vals], 1)
    u, mean, want = _ref(block, two)
    keys, srt, order, s, idx, w = nbr.neighbours(u)
    acc = (w[:, :, None] * mean[np.maximum(idx, 0)]).sum(1)
    assert (2 * acc + w.sum(1)[:, None]).max() >= 1 << 32
    _check(geo, [block, block], [vals, two])


@pytest.mark.gpu
def test_four_channels_cross_1_2_is_version_26_and_decodes_as_version_25(geo):
    rng = np.random.default_rng(257)
    pts = random_cloud(rng, 3000, extent=50, lo=-25)[:, 1:].astype(np.int32)
    base = _colour(rng, pts, 1, np.uint8)
    vals = np.concatenate([base, base + rng.integers(0, 4, (3000, 2)).astype(np.uint8), rng.integers(0, 256, (3000, 1)).astype(np.uint8)], 1)
    for dt in (np.uint8, np.uint16):
        v = vals.astype(dt) * (1 if dt == np.uint8 else 257)
        gb, ab = _check(geo, [pts], [v], cross_channel=(1, 2), masks=[(1, 2)])
        assert ab[0][1] == 26 and ab[0][3] == 4 | (3 << 4)
        assert pkg().GeometryCodec.attr_info(ab[0])["cross_channel"] == (1, 2)
        gp, ap = _check(geo, [pts], [v])
        assert ap[0][1] == 25 and len(ab[0]) < len(ap[0])
        assert np.array_equal(geo.decompress(gb, ab)[1][0], geo.decompress(gp, ap)[1][0])


@pytest.mark.gpu
def test_frames_with_and_without_a_mask_in_one_call(geo):
    """cross_channel=True gives a one-channel frame no mask: versions 25 and 26 in one encode call, and runs of both in
    one decompress"""
    rng = np.random.default_rng(258)
    frames = [random_cloud(rng, n, extent=40, lo=-20)[:, 1:].astype(np.int32) for n in (700, 900, 300, 1100)]
    attrs = [_colour(rng, frames[0], 3, np.uint8), _colour(rng, frames[1], 1, np.uint8), _colour(rng, frames[2], 1, np.uint16)[:, 0],
             _colour(rng, frames[3], 2, np.uint16)]
    gb, ab = _check(geo, frames, attrs, cross_channel=True, masks=[True, None, None, True])
    assert [b[1] for b in ab] == [26, 25, 25, 26]


@pytest.mark.gpu
def test_decode_at_lod_1_2_3_from_the_shortest_prefixes(geo):
    """beside the geometry prefixes; frame 1 has no point of sizes 0 and 1 (coordinates are multiples of 4), so those
    launches of the decoder are skipped at lod 0 and its size classes shift at a level"""
    rng = np.random.default_rng(259)
    G = pkg().GeometryCodec
    frames = [random_cloud(rng, 4000, extent=64, lo=-32)[:, 1:].astype(np.int32),
              random_cloud(rng, 2500, extent=40, lo=-20, stride=4)[:, 1:].astype(np.int32), np.zeros((0, 3), np.int32)]
    assert nbr.neighbours(frames[1])[3].min() == 2
    attrs = [_colour(rng, frames[0], 3, np.uint8), _colour(rng, frames[1], 2, np.uint16), np.zeros((0, 1), np.uint8)]
    for cross, masks in ((False, None), (True, [True, True, None])):
        gb, ab = _check(geo, frames, attrs, cross_channel=cross, masks=masks)
        for k in (1, 2, 3):
            gpre = [b[:G.lod_info(b, k)[0]] for b in gb]
            apre = []
            for f, b in enumerate(ab):
                nbytes, values = G.attr_lod_info(b, k)
                assert (nbytes, values) == nbr.lod_info(b, k) and values == G.lod_info(gb[f], k)[1], (k, f)
                apre.append(b[:nbytes])
            assert len(apre[0]) < len(ab[0])
            cells, vals = geo.decompress(gpre, apre, lod=k)
            for f in (0, 1):
                u, mean, _ = _ref(frames[f], attrs[f])
                wc, wv = _sample(u, mean, k)
                assert np.array_equal(cells[f], wc) and np.array_equal(vals[f], wv), (k, f)
                assert np.array_equal(nbr.decode(apre[f], wc, k)[0], wv), (k, f)
            assert vals[2].shape == (0, 1)
            with pytest.raises(pkg("_abi").PccError):
                geo.decompress(gpre[:1], [apre[0][:-2]], lod=k)


@pytest.mark.gpu
def test_float32_and_device_frames_with_drop_and_index(geo):
    import torch
    rng = np.random.default_rng(260)
    voxel, origin = 0.02, (1.5, -2.0, 0.25)
    lats = [random_cloud(rng, 3000, extent=70, lo=-35)[:, 1:].astype(np.int32)]
    lats.append(np.concatenate([lats[0][:1500], lats[0][:300]]))             # duplicates: merged
    attrs = [_colour(rng, lats[0], 3, np.uint8), _colour(rng, lats[1], 2, np.uint16)]
    want = geo.compress(lats, attributes=attrs, predictor="neighbours", return_index=True)
    for f in (0, 1):
        assert want[1][f] == _ref(lats[f], attrs[f])[2], f
    fl = [(p.astype(np.float32) * np.float32(voxel) + np.asarray(origin, np.float32)).astype(np.float32) for p in lats]
    host = geo.compress(fl, attributes=attrs, predictor="neighbours", voxel=voxel, origin=origin, return_index=True)
    dev = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in fl], attributes=attrs, predictor="neighbours", voxel=voxel,
                       origin=origin, return_index=True)
    assert host[:2] == want[:2] and dev[:2] == want[:2]
    assert all(i.is_cuda and np.array_equal(i.cpu().numpy(), w) and np.array_equal(h, w) for i, h, w in zip(dev[2], host[2], want[2]))
    holes, valid = [f.copy() for f in fl], []
    for f in holes:
        rows = rng.permutation(f.shape[0])[:f.shape[0] // 10]
        f[rows, rng.integers(0, 3, rows.size)] = np.nan
        valid.append(np.isfinite(f).all(axis=1))
    drop = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in holes], attributes=attrs, predictor="neighbours", voxel=voxel,
                        origin=origin, invalid="drop", return_index=True)
    for f in (0, 1):
        assert drop[1][f] == _ref(lats[f][valid[f]], attrs[f][valid[f]])[2], f
        index = drop[2][f].cpu().numpy()
        assert ((index >= 0) == valid[f]).all()
        pts, vals = geo.decompress([drop[0][f]], [drop[1][f]])
        assert np.array_equal(pts[0][index[valid[f]]], lats[f][valid[f]]), f


@pytest.mark.gpu
def test_damaged_blobs_are_refused_or_decode_to_other_values(geo):
    """damaged inputs to a decoder that bounds every index; each is followed by a clean decode in the same process"""
    abi = pkg("_abi")
    rng = np.random.default_rng(261)
    pts = random_cloud(rng, 3000, extent=50, lo=-25)[:, 1:].astype(np.int32)
    vals = _colour(rng, pts, 3, np.uint8)
    gb, ab = _check(geo, [pts], [vals])
    u, mean, _ = _ref(pts, vals)
    blob = ab[0]

    def clean():
        assert np.array_equal(geo.decompress(gb, ab)[1][0], mean)
    head = attr2_ref.HEAD2 + 2 * attr_ref.contexts(1, 3) + 4                 # one chunk
    assert struct.unpack_from("<II", blob, 12 + 64) == (47, 1)
    # one flipped payload word, in a lane's run behind the states and the length table
    word = head + 2 * 192 + 2 * 40
    flipped = blob[:word] + bytes([blob[word] ^ 0x5A, blob[word + 1] ^ 0xA5]) + blob[word + 2:]
    with pytest.raises(abi.PccError) as err:
        geo.decompress(gb, [flipped])
    assert err.value.code == abi.PCC_E_STREAM
    clean()
    # a head whose cells[1] disagrees with the geometry: at lod 1 against the cell count, at lod 0 against the cells' own sizes
    c1 = struct.unpack_from("<I", blob, 16)[0]
    wrong = blob[:16] + struct.pack("<I", c1 - 1) + blob[20:]
    G = pkg().GeometryCodec
    for k in (0, 1):
        with pytest.raises(abi.PccError) as err:
            geo.decompress([gb[0][:G.lod_info(gb[0], k)[0]]], [wrong[:G.attr_lod_info(wrong, k)[0]]], lod=k)
        assert err.value.code == abi.PCC_E_STREAM, k
        clean()
    # the version byte rewritten 25 -> 2: a well-formed version-2 blob of other values
    as2 = blob[:1] + bytes([2]) + blob[2:]
    got = geo.decompress(gb, [as2])[1][0]
    assert got.shape == mean.shape and not np.array_equal(got, mean)
    assert np.array_equal(got, attr2_ref.decode(as2, u)[0])
    clean()
