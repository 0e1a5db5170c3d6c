"""Attribute blob versions 28 and 31 on the GPU (compress(..., attributes=..., predictor="bounded-neighbours",
max_error=e); include/pcc.h has the rule): every encode is compared byte for byte against the numpy restatement
tests/attr_nbr_nl_ref.py, every decode against the restatement's decode and against the e-bound to the lossless values, at
a level of detail against v^ of the Morton-first point of every cell.  Frames stay at 9 000 points and below; a reference
blob is computed once per frame and setting."""
import struct

import numpy as np
import pytest

import attr2_ref
import attr_nbr_nl_ref as nnl
import attr_nbr_ref as nbr
import attr_nl_ref
import attr_ref
from conftest import pkg, random_cloud
from test_geometry_attributes_lod import _sample


@pytest.fixture(scope="module")
def geo():
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _merged(p, a, k=0):
    """the cells p >> k in Morton order and their merged values"""
    a2 = a if a.ndim == 2 else a[:, None]
    u, mean = attr_ref.merge(np.asarray(p, np.int32).reshape(-1, 3) >> k, a2)
    o = np.argsort(attr2_ref.keys_of(u, 32768 >> k))
    return u[o], mean[o]


def _check(geo, frames, attrs, e, cross_channel=False, masks=None, lod=0, decode=True):
    """compress under the keyword: the blobs are the restatement's; they decode to the restatement's values, which lie
    within e of the merged (lossless) values -> (geometry blobs, attribute blobs, the decoded values)"""
    gb, ab = geo.compress(frames, attributes=attrs, predictor="bounded-neighbours", max_error=e, cross_channel=cross_channel, lod=lod)
    assert gb == geo.compress(frames, lod=lod)
    cells, vals = geo.decompress(gb, ab)
    for f, (p, a) in enumerate(zip(frames, attrs)):
        u, mean = _merged(p, a, lod)
        want = nnl.encode(u, mean, a.dtype.itemsize, e, bias=32768 >> lod, cross=None if masks is None else masks[f])
        assert ab[f] == want, f"frame {f}: {len(ab[f])} bytes, the restatement {len(want)}; head {ab[f][:16].hex()} / {want[:16].hex()}"
        assert np.array_equal(cells[f], u) and vals[f].dtype == a.dtype and vals[f].shape == mean.shape, f
        if mean.shape[0]:
            assert np.abs(vals[f].astype(np.int64) - mean).max() <= e, f
        if decode:
            assert np.array_equal(vals[f], nnl.decode(want, u)[0]), f
    return gb, ab, vals


def _colour(rng, pts, c, dtype):
    """smooth in space, so that a predictor has something to find, with noise"""
    top = np.iinfo(dtype).max
    base = (pts.astype(np.int64) * np.array([3, 5, 7])).sum(1)[:, None] * (top // 255) + rng.integers(0, 40 * (top // 255), (pts.shape[0], c))
    return (base % (top + 1)).astype(dtype)


@pytest.fixture(scope="module")
def six():
    """0, 1, 2, 257 (one past a block), 9 000 and 9 000 points; uint8 and uint16; 1, 3 and 4 channels"""
    rng = np.random.default_rng(281)
    frames = [random_cloud(rng, n, extent=60, lo=-30)[:, 1:].astype(np.int32) if n else np.zeros((0, 3), np.int32)
              for n in (0, 1, 2, 257, 9000, 9000)]
    kinds = ((3, np.uint8), (1, np.uint16), (4, np.uint8), (3, np.uint16), (3, np.uint8), (4, np.uint16))
    attrs = [_colour(rng, p, c, dt) for p, (c, dt) in zip(frames, kinds)]
    attrs[1] = attrs[1][:, 0]                                                 # a one-channel frame given as [n]
    return frames, attrs


@pytest.mark.gpu
@pytest.mark.parametrize("e", [1, 2])
def test_six_frames_of_mixed_widths_in_one_call(geo, six, e):
    frames, attrs = six
    gb, ab, vals = _check(geo, frames, attrs, e)
    assert [b[1] for b in ab] == [28] * 6 and len(ab[0]) == 12
    G = pkg().GeometryCodec
    assert G.attr_info(ab[3]) == {"version": 28, "bpv": 2, "channels": 3, "points": 257, "max_error": e, "scalable": True, "lod": 0,
                                  "predictor": "neighbours"}
    assert G.attr_info(ab[0])["predictor"] == "neighbours" and G.attr_info(ab[0])["points"] == 0
    # within e of what the lossless kind decodes, and the setting moves bytes
    gl, al = geo.compress(frames, attributes=attrs, predictor="neighbours")
    lossless = geo.decompress(gl, al)[1]
    for f in range(1, 6):
        assert np.abs(vals[f].astype(np.int64) - lossless[f].astype(np.int64)).max() <= e, f
    assert len(ab[4]) < len(al[4]) and len(ab[5]) < len(al[5])


@pytest.mark.gpu
def test_the_largest_errors_clamp_at_both_ends(geo):
    """uint8 at e = 127 and uint16 at e = 32 767, values placed at 0 and at mask: the restatement's unclamped sums leave
    the range on both sides, so both clamps of encoder and decoder are taken"""
    rng = np.random.default_rng(282)
    pts = random_cloud(rng, 1500, extent=30, lo=-15)[:, 1:].astype(np.int32)
    for dt, e in ((np.uint8, 127), (np.uint16, 32767)):
        mask = int(np.iinfo(dt).max)
        vals = rng.integers(0, mask + 1, (1500, 2)).astype(dt)
        vals[rng.random(vals.shape) < 0.25] = 0
        vals[rng.random(vals.shape) < 0.25] = mask
        u, mean = _merged(pts, vals)
        keys, srt, order, s, idx, w = nbr.neighbours(u)
        j, vh = nnl.closed_loop(mean, s, idx, w, e, mask)
        y = nbr.predict(vh, idx, w) + j * (2 * e + 1)
        assert y.min() < 0 and y.max() > mask and (mean == 0).any() and (mean == mask).any()
        gb, ab, got = _check(geo, [pts], [vals], e)
        assert np.array_equal(got[0], vh) and struct.unpack_from("<I", ab[0], 12)[0] == e


@pytest.mark.gpu
def test_clusters_far_apart_leave_sizes_without_a_point(geo):
    """four clusters of adjacent points, thousands of cells apart: sizes 0 .. 2 inside a cluster, 11 and above between
    them, none between, so the decoder skips those launches and the encoder's grids of those sizes find empty ranges"""
    rng = np.random.default_rng(283)
    g = np.arange(6)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([block + np.array(o) for o in ((-20000, 8, 3000), (4096, 4096, 4096), (16, -9000, 12000), (25000, 25000, -25000))])
    pts = pts[rng.random(pts.shape[0]) < 0.8].astype(np.int32)
    sizes = set(nbr.neighbours(pts)[3].tolist())
    assert {0, 1, 2} <= sizes and not sizes & set(range(4, 11)) and max(sizes - {16}) >= 11
    _check(geo, [pts, pts[:200]], [_colour(rng, pts, 3, np.uint8), _colour(rng, pts[:200], 1, np.uint16)], 2)


@pytest.mark.gpu
def test_cross_channel_true_and_1_2_beside_a_fourth_channel(geo):
    rng = np.random.default_rng(284)
    pts = random_cloud(rng, 3000, extent=50, lo=-25)[:, 1:].astype(np.int32)
    base = _colour(rng, pts, 1, np.uint8)
    vals = np.concatenate([base, base + rng.integers(0, 4, (3000, 2)).astype(np.uint8), rng.integers(0, 256, (3000, 1)).astype(np.uint8)], 1)
    gp, ap, plain = _check(geo, [pts], [vals], 2)
    for dt in (np.uint8, np.uint16):
        v = vals.astype(dt) * (1 if dt == np.uint8 else 257)
        gb, ab, got = _check(geo, [pts], [v], 2, cross_channel=(1, 2), masks=[(1, 2)], decode=dt == np.uint8)
        assert ab[0][1] == 31 and ab[0][3] == 4 | (3 << 4)
        assert pkg().GeometryCodec.attr_info(ab[0])["cross_channel"] == (1, 2)
        if dt == np.uint8:                                                    # the values of the plain form, in fewer bytes
            assert np.array_equal(got[0], plain[0]) and len(ab[0]) < len(ap[0])
    # True: a one-channel frame gets no mask, versions 28 and 31 in one encode call and runs of both in one decompress
    frames = [pts[:700], pts[700:1600], pts[1600:1900]]
    attrs = [vals[:700, :3], vals[700:1600, 0], vals[1600:1900, :2].astype(np.uint16)]
    gb, ab, _ = _check(geo, frames, attrs, 1, cross_channel=True, masks=[True, None, True])
    assert [b[1] for b in ab] == [31, 28, 31]


@pytest.fixture(scope="module")
def one9000():
    rng = np.random.default_rng(285)
    pts = random_cloud(rng, 9000, extent=64, lo=-32)[:, 1:].astype(np.int32)
    return pts, _colour(rng, pts, 3, np.uint8)


@pytest.mark.gpu
def test_decode_at_lod_1_2_3_from_the_shortest_prefixes(geo, one9000):
    """both blobs cut by lod_info / attr_lod_info: the rows are the restatement's (v^ of the Morton-first point of every
    cell, the rows of the whole decode) and lie within e of the lossless kinds' rows"""
    G = pkg().GeometryCodec
    pts, vals = one9000
    e = 2
    gb, ab, whole = _check(geo, [pts], [vals], e)
    u, mean = _merged(pts, vals)
    for k in (1, 2, 3):
        nbytes, values = G.attr_lod_info(ab[0], k)
        assert (nbytes, values) == nnl.lod_info(ab[0], k) and values == G.lod_info(gb[0], k)[1] and nbytes < len(ab[0]), k
        gpre, apre = [gb[0][:G.lod_info(gb[0], k)[0]]], [ab[0][:nbytes]]
        cells, got = geo.decompress(gpre, apre, lod=k)
        wc, wv = _sample(u, mean, k)
        assert np.array_equal(cells[0], wc) and np.array_equal(got[0], _sample(u, whole[0], k)[1]), k
        assert np.array_equal(got[0], nnl.decode(apre[0], wc, k)[0]), k
        assert np.abs(got[0].astype(np.int64) - wv).max() <= e, k
        with pytest.raises(pkg("_abi").PccError):
            geo.decompress(gpre, [apre[0][:-2]], lod=k)


@pytest.mark.gpu
def test_sender_side_lod_2(geo):
    """compress(..., lod=2): the cells' means over the cells' keys, the lattice 65536 >> 2 (sizes 14 and 15 are not
    launched), slod in the head"""
    rng = np.random.default_rng(286)
    pts = random_cloud(rng, 4000, extent=80, lo=-40)[:, 1:].astype(np.int32)
    edge = np.array([[-32768, -32768, -32768], [32767, 32767, 32767], [32764, -32765, 5]], np.int32)
    frames = [pts, np.concatenate([pts[:500], edge])]
    gb, ab, _ = _check(geo, frames, [_colour(rng, p, 3, np.uint8) for p in frames], 2, lod=2)
    assert all(b[1] == 28 and b[2] >> 4 == 2 for b in ab)
    assert pkg().GeometryCodec.attr_info(ab[0])["lod"] == 2


@pytest.mark.gpu
def test_float32_and_device_frames_with_drop_index_and_device_output(geo):
    import torch
    rng = np.random.default_rng(287)
    voxel, origin = 0.02, (1.5, -2.0, 0.25)
    lats = [random_cloud(rng, 3000, extent=70, lo=-35)[:, 1:].astype(np.int32)]
    lats.append(np.concatenate([lats[0][:1500], lats[0][:300]]))             # duplicates: merged
    attrs = [_colour(rng, lats[0], 3, np.uint8), _colour(rng, lats[1], 2, np.uint16)]
    kw = dict(predictor="bounded-neighbours", max_error=2)
    want = geo.compress(lats, attributes=attrs, return_index=True, **kw)
    refs = [nnl.encode(*_merged(lats[f], attrs[f]), attrs[f].dtype.itemsize, 2) for f in (0, 1)]
    assert want[1] == refs
    fl = [(p.astype(np.float32) * np.float32(voxel) + np.asarray(origin, np.float32)).astype(np.float32) for p in lats]
    host = geo.compress(fl, attributes=attrs, voxel=voxel, origin=origin, return_index=True, **kw)
    dev = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in fl], attributes=attrs, voxel=voxel, origin=origin, return_index=True, **kw)
    assert host[:2] == want[:2] and dev[:2] == want[:2]
    assert all(i.is_cuda and np.array_equal(i.cpu().numpy(), w) and np.array_equal(h, w) for i, h, w in zip(dev[2], host[2], want[2]))
    holes, valid = [f.copy() for f in fl], []
    for f in holes:
        rows = rng.permutation(f.shape[0])[:f.shape[0] // 10]
        f[rows, rng.integers(0, 3, rows.size)] = np.nan
        valid.append(np.isfinite(f).all(axis=1))
    drop = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in holes], attributes=attrs, voxel=voxel, origin=origin, invalid="drop",
                        return_index=True, **kw)
    for f in (0, 1):
        assert drop[1][f] == nnl.encode(*_merged(lats[f][valid[f]], attrs[f][valid[f]]), attrs[f].dtype.itemsize, 2), f
        index = drop[2][f].cpu().numpy()
        assert ((index >= 0) == valid[f]).all()
        pts, vals = geo.decompress([drop[0][f]], [drop[1][f]])
        assert np.array_equal(pts[0][index[valid[f]]], lats[f][valid[f]]), f
    # output="device": the same rows as tensors on the codec's device
    pn, vn = geo.decompress(want[0], want[1])
    pd, vd = geo.decompress(want[0], want[1], output="device")
    for f in (0, 1):
        assert vd[f].is_cuda and np.array_equal(vd[f].cpu().numpy(), vn[f]) and np.array_equal(pd[f].cpu().numpy(), pn[f]), f
        assert np.array_equal(vn[f], nnl.decode(refs[f], pn[f])[0]), f


@pytest.mark.gpu
def test_eight_frames_in_one_call_and_eight_calls_of_one(geo):
    rng = np.random.default_rng(288)
    frames = [random_cloud(rng, n, extent=40, lo=-20)[:, 1:].astype(np.int32) for n in (900, 1, 300, 2500, 64, 257, 1200, 2)]
    attrs = [_colour(rng, p, 1 + f % 4, np.uint8 if f % 2 else np.uint16) for f, p in enumerate(frames)]
    kw = dict(predictor="bounded-neighbours", max_error=2, cross_channel=True)
    gb, ab = geo.compress(frames, attributes=attrs, **kw)
    for f in range(8):
        g1, a1 = geo.compress(frames[f:f + 1], attributes=attrs[f:f + 1], **kw)
        assert (g1[0], a1[0]) == (gb[f], ab[f]), f
    assert sorted(set(b[1] for b in ab)) == [28, 31]


@pytest.mark.gpu
def test_the_kinds_of_before_keep_their_bytes_and_mix_at_lod_0(geo, one9000):
    """predictor="neighbours" against attr_nbr_ref, plain max_error=e with and without scalable=True against attr_nl_ref;
    then one decompress over blobs of versions 2, 7, 25, 28 and 31"""
    rng = np.random.default_rng(289)
    pts, vals = one9000[0][:3000], one9000[1][:3000]
    u, mean = _merged(pts, vals)
    g25, a25 = geo.compress([pts], attributes=[vals], predictor="neighbours")
    assert a25[0] == nbr.encode(u, mean, 1)
    g7, a7 = geo.compress([pts], attributes=[vals], max_error=2, scalable=True)
    assert a7[0] == attr_nl_ref.encode(mean, 1, 2, points=u)
    g4, a4 = geo.compress([pts], attributes=[vals], max_error=2)
    assert a4[0] == attr_nl_ref.encode(mean, 1, 2)
    g2, a2 = geo.compress([pts], attributes=[vals], scalable=True)
    assert a2[0] == attr2_ref.encode(u, mean, 1)
    g28, a28 = geo.compress([pts], attributes=[vals], predictor="bounded-neighbours", max_error=2)
    g31, a31 = geo.compress([pts], attributes=[vals], predictor="bounded-neighbours", max_error=2, cross_channel=True, scalable=True)
    assert [b[0][1] for b in (a2, a7, a25, a28, a31)] == [2, 7, 25, 28, 31] and len(a28[0]) < len(a7[0])
    cells, got = geo.decompress(g2 + g7 + g25 + g28 + g31 + g28, a2 + a7 + a25 + a28 + a31 + a28)
    assert np.array_equal(got[0], mean) and np.array_equal(got[2], mean)
    assert np.array_equal(got[1], attr_nl_ref.decode(a7[0], u)[0])
    want = nnl.decode(a28[0], u)[0]
    assert np.array_equal(got[3], want) and np.array_equal(got[4], want) and np.array_equal(got[5], want)
    assert not np.array_equal(got[3], got[1]) and np.abs(got[3].astype(np.int64) - mean).max() <= 2


@pytest.mark.gpu
def test_damaged_blobs_are_refused_or_decode_to_values_in_range(geo):
    """damaged inputs to a decoder that takes no index from the stream; each is followed by a clean decode in the same
    process"""
    abi = pkg("_abi")
    G = pkg().GeometryCodec
    rng = np.random.default_rng(290)
    pts = random_cloud(rng, 3000, extent=50, lo=-25)[:, 1:].astype(np.int32)
    vals = _colour(rng, pts, 3, np.uint8)
    gb, ab, good = _check(geo, [pts], [vals], 2)
    u, mean = _merged(pts, vals)
    blob = ab[0]

    def clean():
        assert np.array_equal(geo.decompress(gb, ab)[1][0], good[0])

    def refused_or_in_range(attr, k=0):
        try:
            got = geo.decompress([gb[0][:G.lod_info(gb[0], k)[0]]], [attr], lod=k)[1][0]
        except abi.PccError as err:
            assert err.code == abi.PCC_E_STREAM
            return None
        assert got.dtype == np.uint8 and got.shape[1] == 3
        return got
    head = attr2_ref.HEAD2 + 4 + 2 * attr_ref.contexts(1, 3) + 4             # one chunk
    assert struct.unpack_from("<II", blob, 16 + 64) == (47, 1)
    # one flipped payload word, in a lane's run behind the states and the length table
    word = head + 2 * 192 + 2 * 40
    assert refused_or_in_range(blob[:word] + bytes([blob[word] ^ 0x5A, blob[word + 1] ^ 0xA5]) + blob[word + 2:]) is None
    clean()
    # a head whose cells[1] disagrees with the geometry: at lod 1 against the cell count, at lod 0 against the cells' own sizes
    c1 = struct.unpack_from("<I", blob, 20)[0]
    wrong = blob[:20] + struct.pack("<I", c1 - 1) + blob[24:]
    for k in (0, 1):
        assert refused_or_in_range(wrong[:G.attr_lod_info(wrong, k)[0]], k) is None, k
        clean()
    # max_error outside 1 .. 2^(8 bpv - 1) - 1: the parser refuses both
    for bad in (0, 128):
        assert refused_or_in_range(blob[:12] + struct.pack("<I", bad) + blob[16:]) is None, bad
        clean()
    # another bound that the head allows: the same indices under q = 9 give other values, in range or refused
    got = refused_or_in_range(blob[:12] + struct.pack("<I", 4) + blob[16:])
    assert got is None or not np.array_equal(got, good[0])
    clean()
    # the version byte rewritten 28 -> 7: a well-formed version-7 blob of the indices, summed along other chains
    as7 = blob[:1] + bytes([7]) + blob[2:]
    got = refused_or_in_range(as7)
    assert got is None or not np.array_equal(got, good[0])
    clean()
