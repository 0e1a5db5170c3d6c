"""Transform-coded attribute blobs with a colour transform and one step per channel, version 21, on the GPU:
compress(..., qstep=(..)) and compress(..., qstep=q, colour="ycocg") against the numpy restatement
tests/attr_colour_ref.py byte for byte, decompress against its decode value for value, several frames in one call, the
sender's side of a level of detail, float32 / device frames with dropped rows, the kind mixed with others in one call,
what is refused, and the calls of before untouched."""
import struct

import numpy as np
import pytest

import attr2_ref
import attr_colour_ref as K
import attr_ref
import attr_transform_ref as T
from conftest import pkg, random_cloud
from test_geometry_attributes import _expected

REF_DECODE_UP_TO = 300      # the restatement's decoder steps through each decision in numpy; above, its reconstruction
                            # (the CPU tests hold the two equal) stands for it


def _colour(rng, n, c, dtype):
    """correlated channels around a slowly moving base, as a camera's colour"""
    top = 1 << (8 * dtype.itemsize)
    step = 1 if dtype.itemsize == 1 else 97
    base = np.cumsum(rng.integers(-9, 10, n)) * step + rng.integers(0, top)
    return ((base[:, None] + rng.integers(-4, 5, (n, c)) * step) % top).astype(dtype)


def _cloud(rng, n):
    return random_cloud(rng, n, extent=48 if n < 5000 else 96, lo=-20)[:, 1:].astype(np.int32)


def _steps(q, c):
    """a setting's steps for a frame of c channels: an integer as it is, three steps with a fourth for an unrelated channel"""
    return q if isinstance(q, int) else tuple(q) + (6,) * (c - len(q))


class _Batch:
    """one dtype's frames, three channels: 1, 2 (split at bit 0 and at bit 47), 63, 64, 65 (one lane run more), 300 and
    5000 points, 64 points cycling through the eight corners of the colour cube along Morton order, an empty frame, a
    frame with duplicate points, and uint8 x 4 at 8192 / 8193 points (one chunk more, and the untouched fourth channel).
    Coded in ONE call per setting where the setting has one step for every channel, else the frames of three and of four
    channels in a call each."""

    def __init__(self, geo, dtype):
        rng = np.random.default_rng(210 + dtype.itemsize)
        self.geo, self.dtype, self.bpv = geo, dtype, dtype.itemsize
        mask = (1 << (8 * dtype.itemsize)) - 1
        cases = [(_cloud(rng, n), _colour(rng, n, 3, dtype)) for n in (1, 63, 64, 65, 300, 5000)]
        cases.append((np.array([[2, 2, 2], [2, 2, 3]], np.int32), _colour(rng, 2, 3, dtype)))
        cases.append((np.array([[0, 5, 5], [-1, 5, 5]], np.int32), _colour(rng, 2, 3, dtype)))
        self.cube = len(cases)
        cases.append((_cloud(rng, 64), None))
        self.empty = len(cases)
        cases.append((np.zeros((0, 3), np.int32), np.zeros((0, 3), dtype)))
        self.dup = len(cases)
        p = _cloud(rng, 900)
        p = np.concatenate([p, p[:300], p[::7]])[rng.permutation(900 + 300 + 129)]
        cases.append((p, _colour(rng, p.shape[0], 3, dtype)))
        self.three = list(range(len(cases)))
        self.four = []
        if dtype.itemsize == 1:
            self.four = [len(cases), len(cases) + 1]
            cases += [(_cloud(rng, n), _colour(rng, n, 4, dtype)) for n in (8192, 8193)]
        self.frames = [p for p, _ in cases]
        self.blobs = geo.compress(self.frames)
        self.pts = geo.decompress(self.blobs)
        # the corners of the colour cube, one after the other along the decoded (Morton) order
        order = np.argsort(attr2_ref.keys_of(self.frames[self.cube]))
        cube = np.zeros((64, 3), dtype)
        k = np.arange(64) % 8
        cube[order] = np.stack([k >> 2 & 1, k >> 1 & 1, k & 1], 1) * mask
        cases[self.cube] = (self.frames[self.cube], cube)
        self.attrs = [a for _, a in cases]
        self.want = [_expected(p, a, d).astype(np.int64) for (p, a), d in zip(cases, self.pts)]
        self._ref = {}

    def ref(self, q, colour, frames=None):
        """(blob, decoded values) of the restatement, computed once per (setting, frame)"""
        out = []
        for f in range(len(self.frames)) if frames is None else frames:
            if (q, colour, f) not in self._ref:
                qf = _steps(q, self.want[f].shape[1])
                blob = K.encode(self.pts[f], self.want[f], self.bpv, qf, colour)
                n = self.want[f].shape[0]
                vals = K.decode(blob, self.pts[f])[0] if n <= REF_DECODE_UP_TO else K.reconstruct(self.pts[f], self.want[f], self.bpv, qf, colour)
                self._ref[q, colour, f] = (blob, vals)
            out.append(self._ref[q, colour, f])
        return out

    def compress(self, q, colour):
        """the batch under one setting -> (geometry blobs, attribute blobs), frame by frame"""
        kw = dict(colour="ycocg") if colour else {}
        if isinstance(q, int):
            return self.geo.compress(self.frames, attributes=self.attrs, qstep=q, **kw)
        gb, ab = self.geo.compress([self.frames[f] for f in self.three], attributes=[self.attrs[f] for f in self.three], qstep=q, **kw)
        if self.four:
            g4, a4 = self.geo.compress([self.frames[f] for f in self.four], attributes=[self.attrs[f] for f in self.four],
                                       qstep=_steps(q, 4), **kw)
            gb, ab = gb + g4, ab + a4
        return gb, ab


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
@pytest.mark.parametrize("setting", [(1, 1), (7, 1), ("H-1", 1), ((3, 9, 17), 0), ((5, 11, 11), 1)],
                         ids=["ycocg-1", "ycocg-7", "ycocg-H-1", "steps-3-9-17", "ycocg-5-11-11"])
def test_parity_with_the_restatement_both_ways(batches, setting, dtype):
    b = batches(dtype)
    geo, G = b.geo, pkg().GeometryCodec
    q, colour = setting
    H = 1 << (8 * b.bpv - 1)
    q = H - 1 if q == "H-1" else q
    gb, ab = b.compress(q, colour)
    assert gb == b.blobs                                                    # the geometry blobs are unaffected
    ref = b.ref(q, colour)
    for f, (got, (want, _)) in enumerate(zip(ab, ref)):
        assert got == want, f"frame {f}: blob differs from the restatement's ({len(got)} vs {len(want)} bytes)"
        assert G.attr_info(got) == K.info(want), f
    assert ab[b.empty] == bytes([ord("A"), 21, b.bpv, 3]) + bytes(8)
    if setting == (1, 1):
        # the corners: Co and Cg reach 0 and mask, the chroma index reaches its clamp and is coded, and the way back
        # passes G = -1 through the second clamp
        x = K.indices(ab[b.cube])
        assert np.abs(x[1:, 1:]).max() == H - 1
        keys = np.sort(attr2_ref.keys_of(b.pts[b.cube]))
        xm = np.zeros_like(x)
        xm[K.order_of(K.sublevels(keys))] = x
        ycc = K.inverse(keys, xm, (1, 1, 1), b.bpv)
        cg2 = 2 * (ycc[:, 2] - H)
        assert ((cg2 + ycc[:, 0] - (cg2 >> 1)) < 0).any()
    for out in ("numpy", "device"):
        pts, vals = geo.decompress(gb, [r[0] for r in ref], output=out)     # the restatement's blobs through the decoder
        for f, v in enumerate(vals):
            p, v = (pts[f], v) if out == "numpy" else (pts[f].cpu().numpy(), v.cpu().numpy())
            assert v.dtype == b.dtype and np.array_equal(p, b.pts[f]), f
            assert np.array_equal(v, ref[f][1]), f"frame {f} ({out}): decoded values differ from the restatement's"


@pytest.mark.gpu
def test_one_call_of_several_frames(batches):
    """300 points, no points, one point, 65 points, and 8193 points of four channels: one call under an integer step
    with colour, and each frame alone gives the same blob; a sequence of steps fits frames of its length only"""
    b = batches("uint8")
    at = [4, b.empty, 0, b.four[1], 3]
    frames, attrs = [b.frames[f] for f in at], [b.attrs[f] for f in at]
    gb, ab = b.geo.compress(frames, attributes=attrs, qstep=7, colour="ycocg")
    assert ab == [r[0] for r in b.ref(7, 1, at)]
    assert [pkg().GeometryCodec.attr_info(x)["qstep"] for x in ab] == [(7,) * 3, (0,) * 3, (7,) * 3, (7,) * 4, (7,) * 3]
    for f, x in zip(at, ab):
        assert b.geo.compress([b.frames[f]], attributes=[b.attrs[f]], qstep=7, colour="ycocg")[1] == [x], f
    vals = b.geo.decompress(gb, ab)[1]
    assert all(np.array_equal(v, r[1]) for v, r in zip(vals, b.ref(7, 1, at)))
    assert vals[1].shape == (0, 3) and vals[2].shape == (1, 3) and vals[3].shape == (8193, 4)
    with pytest.raises(ValueError, match="frame 3: qstep has 3 steps, the frame has 4 channels"):
        b.geo.compress(frames, attributes=attrs, qstep=(7, 7, 7))
    with pytest.raises(ValueError, match="frame 0: qstep has 4 steps, the frame has 3 channels"):
        b.geo.compress(frames, attributes=attrs, qstep=(7, 7, 7, 7), colour="ycocg")
    three = [i for i in range(len(at)) if i != 3]
    got = b.geo.compress([frames[i] for i in three], attributes=[attrs[i] for i in three], qstep=(7, 7, 7), colour="ycocg")[1]
    assert got == [ab[i] for i in three]                                    # equal steps: the integer's blobs


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_the_senders_side_of_a_level_of_detail(batches, dtype):
    """lod = 2 with colour: the cells' means over the cells' keys, bias 32768 >> 2; the decode runs against the decoded cells"""
    b = batches(dtype)
    at = [4, 5, b.dup, b.empty, 0]
    q = (12, 20, 24) if b.bpv == 1 else (900, 1500, 2000)
    frames, attrs = [b.frames[f] for f in at], [b.attrs[f] for f in at]
    gb, ab = b.geo.compress(frames, attributes=attrs, lod=2, qstep=q, colour="ycocg")
    assert gb == b.geo.compress(frames, lod=2)
    cells = b.geo.decompress(gb)
    pts, vals = b.geo.decompress(gb, ab)
    for i, f in enumerate(at):
        means = _expected(frames[i] >> 2, attrs[i], cells[i]).astype(np.int64)
        assert ab[i] == K.encode(cells[i], means, b.bpv, q, 1, 32768 >> 2), f
        assert ab[i][2] == b.bpv | (2 << 4) and pkg().GeometryCodec.attr_info(ab[i])["lod"] == 2
        assert np.array_equal(pts[i], cells[i]) and np.array_equal(vals[i], K.reconstruct(cells[i], means, b.bpv, q, 1, 32768 >> 2)), f


@pytest.mark.gpu
def test_float32_device_frames_drop_and_index(batches):
    import torch
    b = batches("uint8")
    geo = b.geo
    rng = np.random.default_rng(12)
    voxel, origin = 0.05, (1.0, -2.0, 0.5)
    lats = [_cloud(rng, 3000), np.concatenate([b.frames[5][:2000], b.frames[5][:400]])]      # the second with duplicates
    attrs = [_colour(rng, 3000, 3, np.dtype(np.uint8)), _colour(rng, 2400, 4, np.dtype(np.uint16))]
    fl = [(p.astype(np.float32) * np.float32(voxel) + np.asarray(origin, np.float32)).astype(np.float32) for p in lats]
    kw = dict(qstep=20, colour="ycocg")
    want = geo.compress(lats, attributes=attrs, return_index=True, **kw)
    plain = geo.compress(lats, attributes=attrs, return_index=True)
    assert want[0] == plain[0] and all(np.array_equal(x, y) for x, y in zip(want[2], plain[2]))      # return_index is unchanged
    assert [x[1] for x in want[1]] == [21, 21]
    dev = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in fl], attributes=attrs, voxel=voxel, origin=origin,
                       return_index=True, **kw)
    assert dev[0] == want[0] and dev[1] == want[1]
    assert all(i.is_cuda and np.array_equal(i.cpu().numpy(), w) for i, w in zip(dev[2], want[2]))
    holes = [f.copy() for f in fl]                                          # rows without a return are dropped before coding
    valid = []
    for f in holes:
        rows = rng.permutation(f.shape[0])[:f.shape[0] // 10]
        f[rows, rng.integers(0, 3, rows.size)] = np.nan
        valid.append(np.isfinite(f).all(axis=1))
    holes.append(np.full((5, 3), np.nan, np.float32))
    valid.append(np.zeros(5, bool))
    hattrs = attrs + [np.zeros((5, 3), np.uint8)]
    ints = [p[v] for p, v in zip(lats, valid)] + [np.zeros((0, 3), np.int32)]      # the lattice points the kept rows came from
    kept = geo.compress(ints, attributes=[a[v] for a, v in zip(hattrs, valid)], **kw)      # the equivalent integer host call
    for frames in (holes, [torch.from_numpy(f).to(geo.rt.device) for f in holes]):
        drop = geo.compress(frames, attributes=hattrs, voxel=voxel, origin=origin, invalid="drop", return_index=True, **kw)
        assert drop[:2] == kept
        assert all(((np.asarray(i.cpu() if hasattr(i, "cpu") else i) >= 0) == v).all() for i, v in zip(drop[2], valid))
    assert kept[1][2] == bytes([ord("A"), 21, 1, 3]) + bytes(8)
    nothing = geo.compress([holes[2]], attributes=[hattrs[2]], voxel=voxel, origin=origin, invalid="drop", **kw)
    assert nothing[1] == [kept[1][2]]
    pts, vals = geo.decompress(want[0], want[1], voxel=voxel, origin=origin)
    exact = geo.decompress(want[0], want[1])[1]
    assert all(p.dtype == np.float32 for p in pts) and all(np.array_equal(x, y) for x, y in zip(vals, exact))


@pytest.mark.gpu
def test_mixed_kinds_and_refusals(batches):
    abi = pkg("_abi")
    b = batches("uint8")
    geo, G = b.geo, pkg().GeometryCodec
    at = [4, 3, 2, 1, b.dup, 0, b.empty, 5]
    frames, attrs = [b.frames[f] for f in at], [b.attrs[f] for f in at]
    gb = [b.blobs[f] for f in at]
    kinds = {1: geo.compress(frames, attributes=attrs)[1],
             2: geo.compress(frames, attributes=attrs, scalable=True)[1],
             19: geo.compress(frames, attributes=attrs, qstep=9)[1],
             21: geo.compress(frames, attributes=attrs, qstep=9, colour="ycocg")[1],
             "21 plain": geo.compress(frames, attributes=attrs, qstep=(4, 9, 30))[1]}
    alone = {k: geo.decompress(gb, ab)[1] for k, ab in kinds.items()}
    for k, ab in kinds.items():                                             # every kind alone is the restatement's
        if k in (21, "21 plain"):
            ref = b.ref(9, 1, at) if k == 21 else b.ref((4, 9, 30), 0, at)
            assert ab == [r[0] for r in ref] and all(np.array_equal(v, r[1]) for v, r in zip(alone[k], ref)), k
    order = (21, 1, 2, 21, "21 plain", 19, 21, 1)                           # 21 with and without colour side by side, and beside 19
    mix = [kinds[k][i] for i, k in enumerate(order)]
    assert [x[1] for x in mix] == [21, 1, 2, 21, 21, 19, 21, 1]
    for out in ("numpy", "device"):
        pts, vals = geo.decompress(gb, mix, output=out)
        for i, k in enumerate(order):
            p, v = (pts[i], vals[i]) if out == "numpy" else (pts[i].cpu().numpy(), vals[i].cpu().numpy())
            assert np.array_equal(p, b.pts[at[i]]) and np.array_equal(v, alone[k][i]), (out, i, k)
    # no levels of detail
    with pytest.raises(ValueError, match="frame 2: attributes of blob version 21"):
        geo.decompress(gb[:3], [kinds[2][0], kinds[2][1], kinds[21][2]], lod=1)
    with pytest.raises(abi.PccError) as e:
        G.attr_lod_info(kinds[21][0], 1)
    assert e.value.code == abi.PCC_E_ARG
    # another frame's geometry, with another point count
    with pytest.raises(abi.PccError) as e:
        geo.decompress([gb[0], gb[2]], [kinds[21][0], kinds[21][1]])
    assert e.value.code == abi.PCC_E_STREAM and "frame 1:" in str(e.value)
    # the entry points: the run kinds' refuses 21, the lod entry refuses it beside another kind and above lod 0
    with geo._lock, geo.rt as rt:
        cells = rt.octree_decode_frames(gb[:2], device=True, lod=0)
        for blobs_, kw in (([kinds[21][0]], {}), ([kinds[21][0], kinds[2][1]], {"lod": 0, "cells": cells}),
                           ([kinds[2][0], kinds[21][1]], {"lod": 0, "cells": cells}), ([kinds[21][0], kinds[19][1]], {"lod": 0, "cells": cells}),
                           ([kinds[19][0], kinds[21][1]], {"lod": 0, "cells": cells}), ([kinds[21][0]], {"lod": 1, "cells": cells[:1]})):
            with pytest.raises(abi.PccError) as e:
                rt.attr_decode_frames(blobs_, **kw)
            assert e.value.code in (abi.PCC_E_ARG, abi.PCC_E_STREAM)
    # damaged blobs are named, and the codec stays usable
    x = kinds[21][1]
    for what, bad in (("cut", x[:-2]), ("cut head", x[:27]), ("colour 2", x[:12] + struct.pack("<I", 2) + x[16:]),
                      ("q[1] = 0", x[:20] + bytes(4) + x[24:]), ("q[2] = H", x[:24] + struct.pack("<I", 128) + x[28:]),
                      ("version 23", x[:1] + bytes([23]) + x[2:])):
        with pytest.raises(abi.PccError) as e:
            geo.decompress(gb[:3], [kinds[21][0], bad, kinds[21][2]])
        assert e.value.code == abi.PCC_E_STREAM and "frame 1:" in str(e.value), (what, str(e.value))
    assert all(np.array_equal(p, q) for p, q in zip(geo.decompress(gb, kinds[21])[1], alone[21]))
    # the C entry point's own refusals: a step outside 1 .. H - 1, colour outside {0, 1}, the transform with two channels
    two = [a[:, :2].copy() for a in attrs[:2]]
    with geo._lock, geo.rt as rt:
        front = geo._front(rt, geo._check_frames(frames[:2])[0], False, False, None, "test")
        for a, steps, colour in ((attrs[:2], [5, 0, 5], 0), (attrs[:2], [5, 128, 5], 1), (attrs[:2], [5, 5, 5], 2), (two, [5, 5], 1)):
            with pytest.raises(abi.PccError) as e:
                G._encode_attributes(rt, a, gb[:2], front, 0, pkg("runtime").AttrCoding.of(qstep=steps, colour=colour))
            assert e.value.code == abi.PCC_E_ARG and ("frame 0" in str(e.value) or colour == 2), str(e.value)


@pytest.mark.gpu
def test_the_calls_of_before_are_unchanged(batches):
    """an integer qstep without colour is version 19, byte for byte what its restatement writes; the lossless default
    call gives its bytes"""
    for dtype, f in (("uint8", 4), ("uint16", 3)):
        b = batches(dtype)
        got = b.geo.compress([b.frames[f]], attributes=[b.attrs[f]], qstep=7)
        assert got == ([b.blobs[f]], [T.encode(b.pts[f], b.want[f], b.bpv, 7)]), dtype
        assert b.geo.compress([b.frames[f]], attributes=[b.attrs[f]], qstep=7, colour=None) == got
        assert b.geo.compress([b.frames[f]], attributes=[b.attrs[f]]) == ([b.blobs[f]], [attr_ref.encode(b.want[f], b.bpv)]), dtype
        assert b.geo.compress([b.frames[f]], attributes=[b.attrs[f]], qstep=0, colour=None)[1] == [attr_ref.encode(b.want[f], b.bpv)]
