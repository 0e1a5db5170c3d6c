"""Cross-channel attribute blobs, versions 8, 11, 13 and 14, on the GPU: compress(..., cross_channel=...) against the
numpy restatement tests/attr_cross_ref.py byte for byte and both ways, and against the same call without cross_channel
value for value, at lod 0 and from prefixes; the eight kinds in one call; what is refused."""

import numpy as np
import pytest

import attr_cross_ref
from conftest import pkg, random_cloud
from test_geometry_attributes import _expected

KINDS = {8: (False, 0), 11: (True, 0), 13: (False, 2), 14: (True, 2)}      # version: (scalable, max_error)
PLAIN = {8: 1, 11: 2, 13: 4, 14: 7}
SIZES = (1, 2, 63, 64, 65)
REF_DECODE_UP_TO = 11000    # every frame here; the restatement steps through each decision in numpy


def _colour(rng, n, c, dtype):
    """c channels that follow one signal, as a camera's colour does, over the whole value range (so the values wrap)"""
    top = 1 << (8 * dtype.itemsize)
    step = 1 if dtype.itemsize == 1 else 97
    base = np.cumsum(rng.integers(-9, 10, n)) * step + rng.integers(0, top)
    return ((base[:, None] + rng.integers(-4, 5, (n, c)) * step) % top).astype(dtype)


def _cloud(rng, n):
    return random_cloud(rng, n, extent=48 if n < 5000 else 96, lo=-20)[:, 1:].astype(np.int32)


class _Batch:
    """one dtype's frames: every c in 2 .. 4 at the sizes around a wave, the first two-chunk size of c = 3 (64 x 170 + 1)
    and 8193 points of c = 4, an empty frame (c = 3), a frame of one channel and one with duplicate points"""

    def __init__(self, geo, dtype):
        rng = np.random.default_rng(100 + dtype.itemsize)
        self.geo, self.dtype, self.bpv = geo, dtype, dtype.itemsize
        cases = [(_cloud(rng, n), _colour(rng, n, c, dtype)) for c in (2, 3, 4) for n in SIZES]
        cases.append((_cloud(rng, 10881), _colour(rng, 10881, 3, dtype)))
        cases.append((_cloud(rng, 8193), _colour(rng, 8193, 4, dtype)))
        self.empty = len(cases)
        cases.append((np.zeros((0, 3), np.int32), np.zeros((0, 3), dtype)))
        self.one = len(cases)
        cases.append((_cloud(rng, 500), _colour(rng, 500, 1, dtype)[:, 0]))
        self.dup = len(cases)
        p = _cloud(rng, 900)
        p = np.concatenate([p, p[:300], p[::7]])[rng.permutation(900 + 300 + 129)]
        cases.append((p, _colour(rng, p.shape[0], 3, dtype)))
        self.frames = [p for p, _ in cases]
        self.attrs = [a for _, a in cases]
        self.blobs = geo.compress(self.frames)
        self.pts = geo.decompress(self.blobs)
        self.want = [_expected(p, a if a.ndim == 2 else a[:, None], d) for (p, a), d in zip(cases, self.pts)]
        assert self.want[self.dup].shape[0] == 900
        self._plain, self._ref = {}, {}

    def plain(self, ver):
        """(attribute blobs, decoded values) of the call without cross_channel"""
        if ver not in self._plain:
            scalable, e = KINDS[ver]
            gb, ab = self.geo.compress(self.frames, attributes=self.attrs, scalable=scalable, max_error=e)
            assert gb == self.blobs and all(b[1] == PLAIN[ver] for b in ab)
            self._plain[ver] = (ab, self.geo.decompress(gb, ab)[1])
        return self._plain[ver]

    def ref(self, ver, cross=True, frames=None):
        """the restatement's blobs, computed once"""
        scalable, e = KINDS[ver]
        out = []
        for f in range(len(self.frames)) if frames is None else frames:
            key = (ver, cross, f)
            if key not in self._ref:
                c = self.want[f].shape[1]
                m = cross if cross is True or c > 1 else ()                 # one channel: the plain kind
                self._ref[key] = attr_cross_ref.encode(self.want[f], self.bpv, m, e, points=self.pts[f] if scalable else None)
            out.append(self._ref[key])
        return out


@pytest.fixture(scope="module")
def geo():
    g = pkg().GeometryCodec()
    yield g
    g.close()


@pytest.fixture(scope="module")
def batches(geo):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Batch(geo, np.dtype(name))
        return made[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("ver", sorted(KINDS))
def test_parity_with_the_restatement_both_ways(batches, ver, dtype):
    b = batches(dtype)
    geo, G = b.geo, pkg().GeometryCodec
    scalable, e = KINDS[ver]
    gb, ab = geo.compress(b.frames, attributes=b.attrs, scalable=scalable, max_error=e, cross_channel=True)
    assert gb == b.blobs                                                    # the geometry blobs are unaffected
    ref = b.ref(ver)
    plain_ab, plain_vals = b.plain(ver)
    for f, (got, want) in enumerate(zip(ab, ref)):
        assert got == want, f"frame {f}: blob differs from the restatement's ({len(got)} vs {len(want)} bytes)"
        c = b.want[f].shape[1]
        assert got[1] == (ver if c > 1 else PLAIN[ver]) and got[3] == (c | (((1 << (c - 1)) - 1) << 4)), f
        assert G.attr_info(got) == attr_cross_ref.info(want), f
    assert ab[b.empty] == bytes([ord("A"), ver, b.bpv, 0x33]) + bytes(8)
    assert ab[b.one] == plain_ab[b.one] and ab[b.one][1] == PLAIN[ver] and "cross_channel" not in G.attr_info(ab[b.one])
    pts, vals = geo.decompress(gb, ref)                                     # the restatement's blobs through the decoder
    for f, v in enumerate(vals):
        assert v.dtype == b.dtype and np.array_equal(pts[f], b.pts[f]), f
        assert np.array_equal(v, plain_vals[f]), f"frame {f}: decoded values differ from the plain kind's"
        assert e or np.array_equal(v, b.want[f]), f
        if v.shape[0] <= REF_DECODE_UP_TO:
            assert np.array_equal(v, attr_cross_ref.decode(ref[f], *([b.pts[f]] if scalable else []))[0]), f


@pytest.mark.gpu
@pytest.mark.parametrize("ver", sorted(KINDS))
def test_a_sequence_of_channels(batches, ver):
    """cross_channel as a sequence: a single channel, and (1, 2) beside an unrelated fourth channel"""
    b = batches("uint8")
    geo = b.geo
    scalable, e = KINDS[ver]
    for cross, at in (((1,), [3, 4, 8, 9, 13, 14, 16, b.empty]), ((1, 2), [9, 13, 14, 15, 16, b.dup]), ((3,), [12, 14, 16])):
        gb, ab = geo.compress([b.frames[f] for f in at], attributes=[b.attrs[f] for f in at], scalable=scalable, max_error=e,
                              cross_channel=cross)
        assert ab == b.ref(ver, cross, at), cross
        assert all(pkg().GeometryCodec.attr_info(x)["cross_channel"] == cross for x in ab)
        vals = geo.decompress(gb, ab)[1]
        assert all(np.array_equal(v, b.plain(ver)[1][f]) for v, f in zip(vals, at)), cross
    with pytest.raises(ValueError, match="frame 1:"):
        geo.compress([b.frames[14], b.frames[9]], attributes=[b.attrs[14], b.attrs[9]], cross_channel=(3,))
    with pytest.raises(ValueError, match="frame 0:"):
        geo.compress([b.frames[b.one]], attributes=[b.attrs[b.one]], cross_channel=[1])
    for bad in (1, "1", None, (1.5,)):
        with pytest.raises(TypeError):
            geo.compress([b.frames[9]], attributes=[b.attrs[9]], cross_channel=bad)
    with pytest.raises(ValueError, match="attributes"):
        geo.compress([b.frames[9]], cross_channel=True)
    abi = pkg("_abi")
    with pytest.raises(abi.PccError) as err:                                # the C entry point refuses what Python would have caught
        with geo._lock, geo.rt as rt:
            rt.attr_encode_frames(None, [0], [1 | (3 << 8)], [0, 0], [0], None, None, 0, 1, cross=[4])
    assert err.value.code == abi.PCC_E_ARG and "frame 0:" in str(err.value)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("scalable", [False, True])
def test_equal_to_the_plain_call(batches, scalable, dtype):
    """decompress of a cross call is decompress of the same call without cross_channel, array for array: lossless and at
    e = 2, on the host and on the device, and from the shortest prefixes of lod 2 and 5"""
    b = batches(dtype)
    geo, G = b.geo, pkg().GeometryCodec
    for ver in (11, 14) if scalable else (8, 13):
        e = KINDS[ver][1]
        plain_ab, plain_vals = b.plain(ver)
        gb, ab = geo.compress(b.frames, attributes=b.attrs, scalable=scalable, max_error=e, cross_channel=True)
        for out in ("numpy", "device"):
            pts, vals = geo.decompress(gb, ab, output=out)
            for f, (p, v) in enumerate(zip(pts, vals)):
                p, v = (p, v) if out == "numpy" else (p.cpu().numpy(), v.cpu().numpy())
                assert np.array_equal(p, b.pts[f]) and v.dtype == b.dtype and np.array_equal(v, plain_vals[f]), (ver, out, f)
        for k in (2, 5) if scalable else ():
            ginfo = [G.lod_info(x, k) for x in gb]
            ainfo = [G.attr_lod_info(x, k) for x in ab]
            pinfo = [G.attr_lod_info(x, k) for x in plain_ab]
            assert all(a == attr_cross_ref.lod_info(x, k) for a, x in zip(ainfo, ab)), (ver, k)
            assert all(g[1] == a[1] == p[1] for g, a, p in zip(ginfo, ainfo, pinfo)), (ver, k)
            gpre = [x[:n] for x, (n, _) in zip(gb, ginfo)]
            want = geo.decompress(gpre, [x[:n] for x, (n, _) in zip(plain_ab, pinfo)], lod=k)[1]
            for out in ("numpy", "device"):
                cells, vals = geo.decompress(gpre, [x[:n] for x, (n, _) in zip(ab, ainfo)], output=out, lod=k)
                for f, v in enumerate(vals):
                    v = v if out == "numpy" else v.cpu().numpy()
                    assert v.shape == want[f].shape and np.array_equal(v, want[f]), (ver, k, out, f)
            f = 15                                                          # two chunks: the restatement on the prefix
            cells = geo.decompress([gpre[f]], lod=k)[0]
            assert np.array_equal(attr_cross_ref.decode(ab[f][:ainfo[f][0]], cells, k)[0], want[f]), (ver, k)


@pytest.mark.gpu
def test_the_eight_kinds_in_one_call(batches):
    b = batches("uint8")
    geo = b.geo
    kinds = {}
    for ver, (scalable, e) in KINDS.items():
        kinds[ver] = geo.compress(b.frames, attributes=b.attrs, scalable=scalable, max_error=e, cross_channel=True)[1]
        kinds[PLAIN[ver]] = b.plain(ver)[0]
    order = (1, 8, 2, 11, 4, 13, 7, 14)
    at = [f for f in range(len(b.frames)) if f != b.one]                    # one channel has no cross kind
    mix = [kinds[order[i % 8]][f] for i, f in enumerate(at)]
    assert {x[1] for x in mix} == set(order)
    for out in ("numpy", "device"):
        pts, vals = geo.decompress([b.blobs[f] for f in at], mix, output=out)
        for i, f in enumerate(at):
            ver = order[i % 8]
            want = b.plain(ver if ver in KINDS else {v: k for k, v in PLAIN.items()}[ver])[1][f]
            p, v = (pts[i], vals[i]) if out == "numpy" else (pts[i].cpu().numpy(), vals[i].cpu().numpy())
            assert np.array_equal(p, b.pts[f]) and np.array_equal(v, want), (out, f, ver)


@pytest.mark.gpu
def test_kinds_are_refused_where_they_do_not_belong(batches):
    abi = pkg("_abi")
    b = batches("uint8")
    geo, G = b.geo, pkg().GeometryCodec
    f = 9                                                                   # c = 3, 65 points
    one = lambda **kw: geo.compress([b.frames[f]], attributes=[b.attrs[f]], cross_channel=True, **kw)
    gb, ab8 = one()
    ab13, ab11, ab14 = one(max_error=2)[1], one(scalable=True)[1], one(scalable=True, max_error=2)[1]
    assert [x[0][1] for x in (ab8, ab11, ab13, ab14)] == [8, 11, 13, 14]
    for ab, ver in ((ab8, 8), (ab13, 13)):                                  # one predictive stream: no levels of detail
        with pytest.raises(ValueError, match=f"version {ver}"):
            geo.decompress(gb, ab, lod=1)
        with pytest.raises(abi.PccError) as e:
            G.attr_lod_info(ab[0], 1)
        assert e.value.code == abi.PCC_E_ARG
    with pytest.raises(ValueError, match="frame 1:"):
        geo.decompress(gb + gb, ab11 + ab8, lod=2)
    with geo._lock, geo.rt as rt:
        cells = rt.octree_decode_frames(gb + gb, device=True, lod=0)
        for blobs_, kw, code in (([ab11[0]], {}, abi.PCC_E_STREAM),                              # the lod entry point's kinds
                                 ([ab8[0]], {"lod": 0, "cells": cells[:1]}, abi.PCC_E_STREAM),   # and the other's
                                 ([ab8[0], ab13[0]], {}, abi.PCC_E_ARG),                         # one version per call
                                 ([ab1_of(b, f), ab8[0]], {}, abi.PCC_E_ARG),
                                 ([ab13[0], ab1_of(b, f)], {}, abi.PCC_E_ARG),
                                 ([ab11[0], ab14[0]], {"lod": 0, "cells": cells}, abi.PCC_E_ARG),
                                 ([ab14[0], ab11[0]], {"lod": 0, "cells": cells}, abi.PCC_E_ARG)):
            with pytest.raises(abi.PccError) as e:
                rt.attr_decode_frames(blobs_, **kw)
            assert e.value.code == code and ("frame 0:" in str(e.value) or "frame 1:" in str(e.value)), (kw, str(e.value))
    for ver in (3, 5, 6, 9, 10, 12, 15):                                    # the other version bytes stay refused
        with pytest.raises(abi.PccError) as e:
            geo.decompress(gb, [ab8[0][:1] + bytes([ver]) + ab8[0][2:]])
        assert "frame 0:" in str(e.value), ver
    assert all(np.array_equal(x, y) for x, y in zip(geo.decompress(gb, ab8)[1], [b.want[f]]))


def ab1_of(b, f):
    return b.plain(8)[0][f]


@pytest.mark.gpu
def test_float32_device_frames_drop_and_index(batches, wl):
    import torch
    b = batches("uint8")
    geo = b.geo
    rng = np.random.default_rng(12)
    voxel, origin = 0.05, (1.0, -2.0, 0.5)
    lats = [_cloud(rng, 3000), np.concatenate([b.frames[15][:2000], b.frames[15][:400]])]      # the second with duplicates
    attrs = [_colour(rng, 3000, 3, np.dtype(np.uint8)), _colour(rng, 2400, 4, np.dtype(np.uint16))]
    fl = [(p.astype(np.float32) * np.float32(voxel) + np.asarray(origin, np.float32)).astype(np.float32) for p in lats]
    for scalable, e in ((False, 0), (True, 2)):
        kw = dict(scalable=scalable, max_error=e)
        want = geo.compress(lats, attributes=attrs, cross_channel=True, return_index=True, **kw)
        plain = geo.compress(lats, attributes=attrs, return_index=True, **kw)
        assert want[0] == plain[0] and all(np.array_equal(x, y) for x, y in zip(want[2], plain[2]))
        assert [x[1] for x in want[1]] == [{(False, 0): 8, (True, 2): 14}[scalable, e]] * 2
        dev = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in fl], attributes=attrs, cross_channel=True, voxel=voxel,
                           origin=origin, return_index=True, **kw)
        assert dev[0] == want[0] and dev[1] == want[1], scalable
        assert all(i.is_cuda and np.array_equal(i.cpu().numpy(), w) for i, w in zip(dev[2], want[2])), scalable
        holes = [f.copy() for f in fl]                                      # rows without a return are dropped before coding
        valid = []
        for f in holes:
            rows = rng.permutation(f.shape[0])[:f.shape[0] // 10]
            f[rows, rng.integers(0, 3, rows.size)] = np.nan
            valid.append(np.isfinite(f).all(axis=1))
        holes.append(np.full((5, 3), np.nan, np.float32))
        valid.append(np.zeros(5, bool))
        hattrs = attrs + [np.zeros((5, 2), np.uint8)]
        kept = geo.compress([f[v] for f, v in zip(holes, valid)], attributes=[a[v] for a, v in zip(hattrs, valid)], cross_channel=True,
                            voxel=voxel, origin=origin, **kw)
        drop = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in holes], attributes=hattrs, cross_channel=True, voxel=voxel,
                            origin=origin, invalid="drop", return_index=True, **kw)
        assert drop[:2] == kept and all(((i.cpu().numpy() >= 0) == v).all() for i, v in zip(drop[2], valid)), scalable
        assert kept[1][2] == bytes([ord("A"), want[1][0][1], 1, 2 | (1 << 4)]) + bytes(8)
        nothing = geo.compress([holes[2]], attributes=[hattrs[2]], cross_channel=True, voxel=voxel, origin=origin, invalid="drop", **kw)
        assert nothing[1] == [kept[1][2]]
        pts, vals = geo.decompress(want[0], want[1], voxel=voxel, origin=origin)
        exact = geo.decompress(plain[0], plain[1])[1]
        assert all(p.dtype == np.float32 for p in pts) and all(np.array_equal(x, y) for x, y in zip(vals, exact)), scalable


@pytest.mark.gpu
@pytest.mark.parametrize("ver", sorted(KINDS))
def test_corrupt_blobs_are_named_and_the_codec_stays_usable(batches, ver):
    """a flipped bit of the mask nibble and a cut blob in the middle of a run of frames.  The frame has two channels, so
    that every flip leaves no valid mask (0, or a bit at c - 1 and above); of a wider frame a flip may give another valid
    mask, which decodes, to other values, as a flip inside the payload of any kind may."""
    abi = pkg("_abi")
    b = batches("uint8")
    geo = b.geo
    scalable, e = KINDS[ver]
    at = [8, 4, 13]                                                         # c = 3 (64 points), c = 2 (65), c = 4 (64)
    gb, ab = geo.compress([b.frames[f] for f in at], attributes=[b.attrs[f] for f in at], scalable=scalable, max_error=e,
                          cross_channel=True)
    good = geo.decompress(gb, ab)[1]
    x = ab[1]
    assert x[1] == ver and x[3] == 2 | (1 << 4)
    bad = {f"mask bit {i}": x[:3] + bytes([x[3] ^ (16 << i)]) + x[4:] for i in range(4)}
    bad["cut"] = x[:-2]
    bad["cut head"] = x[:15]
    bad["plain version byte, mask left"] = x[:1] + bytes([PLAIN[ver]]) + x[2:]
    for what, nb in bad.items():
        with pytest.raises(abi.PccError) as err:
            geo.decompress(gb, [ab[0], nb, ab[2]])
        assert err.value.code == abi.PCC_E_STREAM and "frame 1:" in str(err.value), (what, str(err.value))
        again = geo.decompress(gb, ab)[1]                                   # the next call on the same instance
        assert all(np.array_equal(p, q) for p, q in zip(again, good)), what
    if scalable:                                                            # the same through a prefix at lod 1
        G = pkg().GeometryCodec
        gpre = [g[:G.lod_info(g, 1)[0]] for g in gb]
        apre = [a[:G.attr_lod_info(a, 1)[0]] for a in ab]
        good1 = geo.decompress(gpre, apre, lod=1)[1]
        pre = apre[1]
        for what, nb in [(f"mask bit {i}", pre[:3] + bytes([pre[3] ^ (16 << i)]) + pre[4:]) for i in range(4)] + [("two bytes short", pre[:-2])]:
            with pytest.raises(abi.PccError) as err:
                geo.decompress(gpre, [apre[0], nb, apre[2]], lod=1)
            assert "frame 1:" in str(err.value), (what, str(err.value))
            again = geo.decompress(gpre, apre, lod=1)[1]
            assert all(np.array_equal(p, q) for p, q in zip(again, good1)), what


@pytest.mark.gpu
def test_the_default_call_is_unchanged(batches):
    for dtype in ("uint8", "uint16"):
        b = batches(dtype)
        for ver, (scalable, e) in KINDS.items():
            kw = dict(scalable=scalable, max_error=e)
            want = (b.blobs, b.plain(ver)[0])
            assert b.geo.compress(b.frames, attributes=b.attrs, **kw) == want
            assert b.geo.compress(b.frames, attributes=b.attrs, cross_channel=False, **kw) == want
            assert b.geo.compress(b.frames, attributes=b.attrs, cross_channel=(), **kw) == want      # no channel named
        assert [x[1] for x in b.geo.compress(b.frames, attributes=b.attrs)[1]] == [1] * len(b.frames)
