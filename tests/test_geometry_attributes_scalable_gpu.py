"""Transform-coded attribute blobs with level-of-detail prefixes, version 22, on the GPU: compress(..., qstep=..,
scalable_to=K) against the numpy restatement tests/attr_scalable_ref.py byte for byte, decompress at every lod 0 .. K
from the prefixes lod_info / attr_lod_info name against its values, at the shapes where the kernels can go wrong: one
and two points, one K-cell, one point per K-cell, keys that use bit 47, counts around a lane's and a chunk's end, the
index clamp, four channels with colour, K = 1 and K = 5, a sender at lod s with s + K = 15, an empty frame between
others, float32 / device frames with dropped rows, device output, the kind mixed with others, and what is refused."""
import struct

import numpy as np
import pytest

import attr2_ref
import attr_scalable_ref as S
import attr_transform_ref as T
from conftest import pkg, random_cloud
from test_geometry_attributes import _expected

REF_DECODE_UP_TO = 300      # the restatement's entropy decoder steps through each decision in numpy; above, its
                            # reconstruction (the CPU tests hold the two equal) stands for it


def _colour(rng, n, c, dtype):
    top = 1 << (8 * dtype.itemsize)
    step = 1 if dtype.itemsize == 1 else 97
    base = np.cumsum(rng.integers(-9, 10, n)) * step + rng.integers(0, top)
    return ((base[:, None] + rng.integers(-4, 5, (n, c)) * step) % top).astype(dtype)


def _cloud(rng, n, extent=40):
    return random_cloud(rng, n, extent=extent, lo=-extent // 2)[:, 1:].astype(np.int32)


@pytest.fixture(scope="module")
def geo():
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _cells(points, j):
    """the distinct cells points >> j in Morton order"""
    c = np.asarray(points, np.int64) >> j
    keys, first = np.unique(attr2_ref.keys_of(c), return_index=True)
    return c[first].astype(np.int32)


def _both_ways(geo, frames, attrs, q, K, colour=0, slod=0, outputs=("numpy",)):
    """one compress call of the frames; every blob is the restatement's; every lod 0 .. K decodes from the prefixes to the
    restatement's values.  Returns (geometry blobs, attribute blobs)"""
    G = pkg().GeometryCodec
    kw = dict(colour="ycocg") if colour else {}
    gb, ab = geo.compress(frames, attributes=attrs, qstep=q, scalable_to=K, lod=slod, **kw)
    assert gb == geo.compress(frames, lod=slod)                               # the geometry blobs are unaffected
    cells0 = geo.decompress(gb)
    means = []
    for f, (p, a) in enumerate(zip(frames, attrs)):
        bpv = a.dtype.itemsize
        a2 = a if a.ndim == 2 else a[:, None]
        m = _expected(p >> slod, a2, cells0[f]).astype(np.int64)
        means.append(m)
        qf = q if isinstance(q, int) else tuple(q)[:a2.shape[1]]
        want = S.encode(cells0[f], m, bpv, qf, K, colour, 32768 >> slod)
        assert ab[f] == want, f"frame {f}: blob differs from the restatement's ({len(ab[f])} vs {len(want)} bytes)"
        assert G.attr_info(ab[f]) == S.info(want), f
    for j in range(K + 1):
        gp = [b[:G.lod_info(b, j)[0]] for b in gb]
        for f, a in enumerate(ab):
            assert G.attr_lod_info(a, j) == S.lod_info(a, j), (f, j)
        ap = [a[:G.attr_lod_info(a, j)[0]] for a in ab]
        for out in outputs:
            pts, vals = geo.decompress(gp, ap, lod=j, output=out)
            for f, v in enumerate(vals):
                p, v = (pts[f], v) if out == "numpy" else (pts[f].cpu().numpy(), v.cpu().numpy())
                bpv = attrs[f].dtype.itemsize
                qf = q if isinstance(q, int) else tuple(q)[:means[f].shape[1]]
                assert v.dtype == attrs[f].dtype and np.array_equal(p, _cells(cells0[f], j)), (f, j)
                want = S.reconstruct(cells0[f], means[f], bpv, qf, K, colour, 32768 >> slod, lod=j)
                assert np.array_equal(v, want), f"frame {f}, lod {j} ({out}): decoded values differ from the restatement's"
                if 0 < p.shape[0] <= REF_DECODE_UP_TO:
                    assert np.array_equal(S.decode(ap[f], p, j)[0], want), (f, j)
    return gb, ab


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5])
def test_few_points_and_bit_47(geo, K):
    """one point; two points split at bit 0 and at bit 47; the corners -32768 and 32767 in one frame"""
    rng = np.random.default_rng(220 + K)
    frames = [np.array([[3, -4, 5]], np.int32), np.array([[2, 2, 2], [2, 2, 3]], np.int32), np.array([[0, 5, 5], [-1, 5, 5]], np.int32),
              np.array([[-32768, -32768, -32768], [32767, 32767, 32767], [-32768, 32767, 0], [5, 5, 5], [5, 5, 4]], np.int32)]
    attrs = [_colour(rng, p.shape[0], 3, np.dtype(np.uint8)) for p in frames]
    _both_ways(geo, frames, attrs, 6, K, colour=1)
    _both_ways(geo, frames, attrs, (3, 9, 17), K)


@pytest.mark.gpu
def test_one_k_cell_and_one_point_per_k_cell(geo):
    """K = 3: 300 points inside one 8 x 8 x 8 cell (no pair at t >= 9, M = n) and 300 points on multiples of 8 (every
    K-cell holds one point, M = 1, no pair below 9); a frame with sublevels 8 and 9 both occupied beside them"""
    rng = np.random.default_rng(223)
    inside = _cloud(rng, 300, extent=8) + 4 + 64
    apart = _cloud(rng, 300, extent=16) * 8
    both = _cloud(rng, 700)
    for p, (below, above) in ((inside, (True, False)), (apart, (False, True)), (both, (True, True))):
        b = T.sublevels(np.sort(attr2_ref.keys_of(p)))[1:]
        assert ((b < 9).any(), (b >= 9).any()) == (below, above)
    assert (T.sublevels(np.sort(attr2_ref.keys_of(both))) == 8).any() and (T.sublevels(np.sort(attr2_ref.keys_of(both))) == 9).any()
    frames = [inside, apart, both]
    _both_ways(geo, frames, [_colour(rng, p.shape[0], 3, np.dtype(np.uint8)) for p in frames], 9, 3, outputs=("numpy", "device"))
    _both_ways(geo, frames, [_colour(rng, p.shape[0], 1, np.dtype(np.uint16))[:, 0] for p in frames], 700, 3)


@pytest.mark.gpu
def test_lane_and_chunk_ends_and_four_channels_with_colour(geo):
    """64 S - 1, 64 S and 64 S + 1 points for S = 5 (one more point per lane), and 8193 points of four channels (one chunk
    more than 8192; the fourth channel outside the colour transform)"""
    rng = np.random.default_rng(224)
    frames = [_cloud(rng, n) for n in (319, 320, 321)]
    attrs = [_colour(rng, p.shape[0], 3, np.dtype(np.uint8)) for p in frames]
    _both_ways(geo, frames, attrs, 12, 2, colour=1)
    big = [_cloud(rng, 8193, extent=64)]
    _both_ways(geo, big, [_colour(rng, 8193, 4, np.dtype(np.uint8))], (10, 14, 14, 5), 2, colour=1)


@pytest.mark.gpu
def test_the_index_clamp_in_uint16(geo):
    """values 0 and 65535 alternating along Morton order under q = 1 ... H - 1: differences of a full value width"""
    rng = np.random.default_rng(225)
    p = _cloud(rng, 500)
    order = np.argsort(attr2_ref.keys_of(p))
    a = np.zeros((500, 3), np.uint16)
    a[order[1::2]] = 65535
    a[order[::3], 1] = 65535
    gb, ab = _both_ways(geo, [p], [a], 32767, 2)
    gb, ab = _both_ways(geo, [p], [a], 1, 2)
    assert np.abs(S.indices(ab[0], 500)[1:]).max() == 32767                     # the clamp is reached and coded


@pytest.mark.gpu
def test_a_sender_at_lod_10_with_k_5_and_an_empty_frame_in_the_middle(geo):
    rng = np.random.default_rng(226)
    wide = rng.integers(-32768, 32768, (3000, 3)).astype(np.int32)
    frames = [wide, np.zeros((0, 3), np.int32), wide[:700] // 2]
    attrs = [_colour(rng, p.shape[0], 3, np.dtype(np.uint8)) for p in frames]
    gb, ab = _both_ways(geo, frames, attrs, 10, 5, colour=1, slod=10)
    assert ab[1] == bytes([ord("A"), 22, 1 | (10 << 4), 3]) + bytes(8)
    assert [pkg().GeometryCodec.attr_info(x)["scalable_to"] for x in ab] == [5, 0, 5]
    for f in (0, 2):
        assert geo.compress([frames[f]], attributes=[attrs[f]], qstep=10, colour="ycocg", scalable_to=5, lod=10)[1] == [ab[f]]
    gb, ab = _both_ways(geo, [p for p in frames], attrs, 10, 2)             # at lod 0, the empty frame still in the middle
    assert ab[1] == bytes([ord("A"), 22, 1, 3]) + bytes(8)


@pytest.mark.gpu
def test_float32_device_frames_drop_and_index(geo):
    import torch
    rng = np.random.default_rng(227)
    voxel, origin = 0.05, (1.0, -2.0, 0.5)
    base = _cloud(rng, 2000)
    lats = [_cloud(rng, 3000, extent=48), np.concatenate([base, base[:400]])]      # the second with duplicates
    attrs = [_colour(rng, 3000, 3, np.dtype(np.uint8)), _colour(rng, 2400, 4, np.dtype(np.uint16))]
    fl = [(p.astype(np.float32) * np.float32(voxel) + np.asarray(origin, np.float32)).astype(np.float32) for p in lats]
    kw = dict(qstep=20, colour="ycocg", scalable_to=2)
    want = geo.compress(lats, attributes=attrs, return_index=True, **kw)
    plain = geo.compress(lats, attributes=attrs, return_index=True)
    assert want[0] == plain[0] and all(np.array_equal(x, y) for x, y in zip(want[2], plain[2]))
    assert [x[1] for x in want[1]] == [22, 22]
    dev = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in fl], attributes=attrs, voxel=voxel, origin=origin,
                       return_index=True, **kw)
    assert dev[0] == want[0] and dev[1] == want[1]
    assert all(i.is_cuda and np.array_equal(i.cpu().numpy(), w) for i, w in zip(dev[2], want[2]))
    holes, valid = [f.copy() for f in fl], []
    for f in holes:
        rows = rng.permutation(f.shape[0])[:f.shape[0] // 10]
        f[rows, rng.integers(0, 3, rows.size)] = np.nan
        valid.append(np.isfinite(f).all(axis=1))
    holes.append(np.full((5, 3), np.nan, np.float32))
    valid.append(np.zeros(5, bool))
    hattrs = attrs + [np.zeros((5, 3), np.uint8)]
    ints = [p[v] for p, v in zip(lats, valid)] + [np.zeros((0, 3), np.int32)]
    kept = geo.compress(ints, attributes=[a[v] for a, v in zip(hattrs, valid)], **kw)
    for frames in (holes, [torch.from_numpy(f).to(geo.rt.device) for f in holes]):
        drop = geo.compress(frames, attributes=hattrs, voxel=voxel, origin=origin, invalid="drop", return_index=True, **kw)
        assert drop[:2] == kept
        assert all(((np.asarray(i.cpu() if hasattr(i, "cpu") else i) >= 0) == v).all() for i, v in zip(drop[2], valid))
    assert kept[1][2] == bytes([ord("A"), 22, 1, 3]) + bytes(8)
    nothing = geo.compress([holes[2]], attributes=[hattrs[2]], voxel=voxel, origin=origin, invalid="drop", **kw)
    assert nothing[1] == [kept[1][2]]                                       # a call none of whose rows is coded
    G = pkg().GeometryCodec
    gp, ap = [b[:G.lod_info(b, 2)[0]] for b in want[0]], [a[:G.attr_lod_info(a, 2)[0]] for a in want[1]]
    pts, vals = geo.decompress(gp, ap, lod=2, voxel=voxel, origin=origin)
    exact = geo.decompress(gp, ap, lod=2)[1]
    assert all(p.dtype == np.float32 for p in pts) and all(np.array_equal(x, y) for x, y in zip(vals, exact))


@pytest.mark.gpu
def test_mixed_kinds_and_refusals(geo):
    abi = pkg("_abi")
    G = pkg().GeometryCodec
    rng = np.random.default_rng(228)
    frames = [_cloud(rng, n) for n in (300, 65, 1, 700)] + [np.zeros((0, 3), np.int32)]
    attrs = [_colour(rng, p.shape[0], 3, np.dtype(np.uint8)) for p in frames]
    gb = geo.compress(frames)
    kinds = {2: geo.compress(frames, attributes=attrs, scalable=True)[1],
             21: geo.compress(frames, attributes=attrs, qstep=9, colour="ycocg")[1],
             22: geo.compress(frames, attributes=attrs, qstep=9, colour="ycocg", scalable_to=2)[1],
             "22 K=1": geo.compress(frames, attributes=attrs, qstep=9, scalable_to=1)[1]}
    alone = {k: geo.decompress(gb, ab)[1] for k, ab in kinds.items()}
    order = (22, 2, 21, "22 K=1", 22)
    mix = [kinds[k][i] for i, k in enumerate(order)]
    assert [x[1] for x in mix] == [22, 2, 21, 22, 22]
    for out in ("numpy", "device"):
        vals = geo.decompress(gb, mix, output=out)[1]
        for i, k in enumerate(order):
            v = vals[i] if out == "numpy" else vals[i].cpu().numpy()
            assert np.array_equal(v, alone[k][i]), (out, i, k)
    # one call of blobs with different K, each under its own; at lod 1 kinds 2 and 22 side by side
    two = [kinds[22][0], kinds["22 K=1"][1], kinds[2][2], kinds[22][3], kinds[2][4]]
    gp = [b[:G.lod_info(b, 1)[0]] for b in gb]
    vals = geo.decompress(gp, [a[:G.attr_lod_info(a, 1)[0]] for a in two], lod=1)[1]
    for i, k in enumerate((22, "22 K=1", 2, 22, 2)):
        assert np.array_equal(vals[i], geo.decompress([gp[i]], [kinds[k][i]], lod=1)[1][0]), i
    # above K: the API names frame and K, pcc_attr_lod_info and the entry point answer PCC_E_ARG
    with pytest.raises(ValueError, match="frame 1: attributes of blob version 22 with scalable_to = 1 cannot be decoded at lod 2"):
        geo.decompress(gb[:2], [kinds[22][0], kinds["22 K=1"][1]], lod=2)
    with pytest.raises(abi.PccError) as e:
        G.attr_lod_info(kinds[22][0], 3)
    assert e.value.code == abi.PCC_E_ARG
    assert G.attr_lod_info(kinds[22][4], 7) == (12, 0)                          # a blob without points records no K
    with geo._lock, geo.rt as rt:
        cells = rt.octree_decode_frames(gb[:2], device=True, lod=3)
        with pytest.raises(abi.PccError) as e:
            rt.attr_decode_frames(kinds[22][:2], lod=3, cells=cells)
        assert e.value.code == abi.PCC_E_ARG
        cells = rt.octree_decode_frames(gb[:2], device=True, lod=0)
        for blobs_, kw in (([kinds[22][0]], {}), ([kinds[22][0], kinds[21][1]], {"lod": 0, "cells": cells}),
                           ([kinds[2][0], kinds[22][1]], {"lod": 0, "cells": cells})):
            with pytest.raises(abi.PccError) as e:
                rt.attr_decode_frames(blobs_, **kw)
            assert e.value.code in (abi.PCC_E_ARG, abi.PCC_E_STREAM)
    # versions 19 and 21 keep their refusal at lod > 0
    with pytest.raises(ValueError, match="frame 1: attributes of blob version 21"):
        geo.decompress(gp[:2], [kinds[22][0], kinds[21][1]], lod=1)
    # another frame's geometry: another count of cells, or the same count with other K-cells
    with pytest.raises(abi.PccError) as e:
        geo.decompress([gb[0], gb[3]], [kinds[22][0], kinds[22][1]])
    assert e.value.code == abi.PCC_E_STREAM and "frame 1:" in str(e.value)
    other = _cloud(np.random.default_rng(5), 300)
    with pytest.raises(abi.PccError) as e:
        geo.decompress(geo.compress([other]), [kinds[22][0]])
    assert e.value.code == abi.PCC_E_STREAM and "frame 0:" in str(e.value)
    # damaged heads are named, and the codec stays usable
    x = kinds[22][0]
    at_k = 12 + 4 + 12
    for what, bad in (("cut", x[:-2]), ("cut head", x[:at_k + 2]), ("K = 0", x[:at_k] + bytes(4) + x[at_k + 4:]),
                      ("K = 16", x[:at_k] + struct.pack("<I", 16) + x[at_k + 4:]),
                      ("count[2] + 1", x[:at_k + 12] + struct.pack("<I", struct.unpack_from("<I", x, at_k + 12)[0] + 1) + x[at_k + 16:]),
                      ("colour 2", x[:12] + struct.pack("<I", 2) + x[16:])):
        with pytest.raises(abi.PccError) as e:
            geo.decompress(gb[:2], [bad, kinds[22][1]])
        assert e.value.code == abi.PCC_E_STREAM and "frame 0:" in str(e.value), (what, str(e.value))
    assert all(np.array_equal(p, q) for p, q in zip(geo.decompress(gb, kinds[22])[1], alone[22]))
    # the C entry point's own refusals: K of 0, and K beyond 15 - key_shift / 3
    with geo._lock, geo.rt as rt:
        front = geo._front(rt, geo._check_frames(frames[:2])[0], False, False, None, "test")
        for key_shift, K in ((0, 0), (0, 16), (3 * 11, 5)):
            with pytest.raises(abi.PccError) as e:
                G._encode_attributes(rt, attrs[:2], gb[:2], front, key_shift, pkg("runtime").AttrCoding.of(qstep=[5, 5, 5], colour=0, scalable_to=K))
            assert e.value.code == abi.PCC_E_ARG, str(e.value)


@pytest.mark.gpu
def test_the_calls_of_before_are_unchanged(geo):
    import attr_colour_ref as C21
    import attr_ref
    rng = np.random.default_rng(229)
    p, a = _cloud(rng, 700), _colour(rng, 700, 3, np.dtype(np.uint8))
    gb = geo.compress([p])
    pts = geo.decompress(gb)[0]
    want = _expected(p, a, pts).astype(np.int64)
    assert geo.compress([p], attributes=[a], qstep=7, scalable_to=None)[1] == [T.encode(pts, want, 1, 7)]
    assert geo.compress([p], attributes=[a], qstep=7, colour="ycocg", scalable_to=None)[1] == [C21.encode(pts, want, 1, 7, 1)]
    assert geo.compress([p], attributes=[a], scalable_to=None)[1] == [attr_ref.encode(want, 1)]
