"""Transform-coded attribute blobs, version 19, on the GPU: compress(..., qstep=q) against the numpy restatement
tests/attr_transform_ref.py byte for byte, decompress against its decode value for value, the sender's side of a level
of detail, float32 / device frames with dropped rows, the kind mixed with others in one call, what is refused, one
recorded frame through distortion(), and the default calls untouched."""
import os

import numpy as np
import pytest

import attr2_ref
import attr_cross_ref
import attr_nl_ref
import attr_ref
import attr_transform_ref as T
from conftest import ROOT, pkg, random_cloud
from test_geometry_attributes import _expected

REF_DECODE_UP_TO = 300      # the restatement's decoder steps through each decision in numpy; above, its reconstruction
                            # (the CPU tests hold the two equal) stands for it


def _colour(rng, n, c, dtype):
    top = 1 << (8 * dtype.itemsize)
    step = 1 if dtype.itemsize == 1 else 97
    base = np.cumsum(rng.integers(-9, 10, n)) * step + rng.integers(0, top)
    return ((base[:, None] + rng.integers(-4, 5, (n, c)) * step) % top).astype(dtype)


def _cloud(rng, n):
    return random_cloud(rng, n, extent=48 if n < 5000 else 96, lo=-20)[:, 1:].astype(np.int32)


class _Batch:
    """one dtype's frames, coded in ONE call per q: uint8 x 3 / uint16 x 2 at 1, 2 (split at bit 0 and at bit 47), 63, 64,
    65 (one lane run more), 300 and 5000 points, 64 values alternating 0 / mask (the clamp of the index), an empty frame,
    a frame with duplicate points, and uint8 x 4 at 8192 / 8193 points (one chunk more)"""

    def __init__(self, geo, dtype):
        rng = np.random.default_rng(190 + dtype.itemsize)
        self.geo, self.dtype, self.bpv = geo, dtype, dtype.itemsize
        c = 3 if dtype.itemsize == 1 else 2
        mask = (1 << (8 * dtype.itemsize)) - 1
        cases = [(_cloud(rng, n), _colour(rng, n, c, dtype)) for n in (1, 63, 64, 65, 300, 5000)]
        cases.append((np.array([[2, 2, 2], [2, 2, 3]], np.int32), _colour(rng, 2, c, dtype)))
        cases.append((np.array([[0, 5, 5], [-1, 5, 5]], np.int32), _colour(rng, 2, c, dtype)))
        self.alt = len(cases)
        cases.append((_cloud(rng, 64), None))
        self.empty = len(cases)
        cases.append((np.zeros((0, 3), np.int32), np.zeros((0, c), dtype)))
        self.dup = len(cases)
        p = _cloud(rng, 900)
        p = np.concatenate([p, p[:300], p[::7]])[rng.permutation(900 + 300 + 129)]
        cases.append((p, _colour(rng, p.shape[0], c, dtype)))
        if dtype.itemsize == 1:
            cases += [(_cloud(rng, n), _colour(rng, n, 4, dtype)) for n in (8192, 8193)]
        self.frames = [p for p, _ in cases]
        self.blobs = geo.compress(self.frames)
        self.pts = geo.decompress(self.blobs)
        # the alternating frame: 0 / mask along the decoded (Morton) order
        order = np.argsort(attr2_ref.keys_of(self.frames[self.alt]))
        alt = np.zeros((64, 1), dtype)
        alt[order, 0] = (np.arange(64) % 2) * mask
        cases[self.alt] = (self.frames[self.alt], alt)
        self.attrs = [a for _, a in cases]
        self.want = [_expected(p, a, d).astype(np.int64) for (p, a), d in zip(cases, self.pts)]
        self._ref = {}

    def ref(self, q, frames=None):
        """(blob, decoded values) of the restatement, computed once per (q, frame)"""
        out = []
        for f in range(len(self.frames)) if frames is None else frames:
            if (q, f) not in self._ref:
                blob = T.encode(self.pts[f], self.want[f], self.bpv, q)
                n = self.want[f].shape[0]
                vals = T.decode(blob, self.pts[f])[0] if n <= REF_DECODE_UP_TO else T.reconstruct(self.pts[f], self.want[f], self.bpv, q)
                self._ref[q, f] = (blob, vals)
            out.append(self._ref[q, f])
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
@pytest.mark.parametrize("q", [1, 7, "H-1"])
def test_parity_with_the_restatement_both_ways(batches, q, dtype):
    b = batches(dtype)
    geo, G = b.geo, pkg().GeometryCodec
    q = (1 << (8 * b.bpv - 1)) - 1 if q == "H-1" else q
    gb, ab = geo.compress(b.frames, attributes=b.attrs, qstep=q)
    assert gb == b.blobs                                                    # the geometry blobs are unaffected
    ref = b.ref(q)
    for f, (got, (want, _)) in enumerate(zip(ab, ref)):
        assert got == want, f"frame {f}: blob differs from the restatement's ({len(got)} vs {len(want)} bytes)"
        assert G.attr_info(got) == T.info(want), f
    assert ab[b.empty] == bytes([ord("A"), 19, b.bpv, b.attrs[b.empty].shape[1]]) + bytes(8)
    if q == 1:                                                              # the clamp of the index is reached and coded
        assert np.abs(T.indices(ab[b.alt])[1:]).max() == (1 << (8 * b.bpv - 1)) - 1
    for out in ("numpy", "device"):
        pts, vals = geo.decompress(gb, [r[0] for r in ref], output=out)     # the restatement's blobs through the decoder
        for f, v in enumerate(vals):
            p, v = (pts[f], v) if out == "numpy" else (pts[f].cpu().numpy(), v.cpu().numpy())
            assert v.dtype == b.dtype and np.array_equal(p, b.pts[f]), f
            assert np.array_equal(v, ref[f][1]), f"frame {f} ({out}): decoded values differ from the restatement's"


@pytest.mark.gpu
def test_one_call_of_four_frames(batches):
    """300 points, no points, one point, 65 points: one call, and each frame alone gives the same blob"""
    b = batches("uint8")
    at = [4, b.empty, 0, 3]
    gb, ab = b.geo.compress([b.frames[f] for f in at], attributes=[b.attrs[f] for f in at], qstep=7)
    assert ab == [r[0] for r in b.ref(7, at)]
    for f, x in zip(at, ab):
        assert b.geo.compress([b.frames[f]], attributes=[b.attrs[f]], qstep=7)[1] == [x], f
    vals = b.geo.decompress(gb, ab)[1]
    assert all(np.array_equal(v, r[1]) for v, r in zip(vals, b.ref(7, at)))
    assert vals[1].shape == (0, 3) and vals[2].shape == (1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_the_senders_side_of_a_level_of_detail(batches, dtype):
    """lod = 2: the cells' means over the cells' keys, bias 32768 >> 2; the decode runs against the decoded cells"""
    b = batches(dtype)
    at = [4, 5, b.dup, b.empty, 0]
    q = 12 if b.bpv == 1 else 900
    frames, attrs = [b.frames[f] for f in at], [b.attrs[f] for f in at]
    gb, ab = b.geo.compress(frames, attributes=attrs, lod=2, qstep=q)
    assert gb == b.geo.compress(frames, lod=2)
    cells = b.geo.decompress(gb)
    pts, vals = b.geo.decompress(gb, ab)
    for i, f in enumerate(at):
        means = _expected(frames[i] >> 2, attrs[i], cells[i]).astype(np.int64)
        assert ab[i] == T.encode(cells[i], means, b.bpv, q, 32768 >> 2), f
        assert ab[i][2] == b.bpv | (2 << 4) and pkg().GeometryCodec.attr_info(ab[i])["lod"] == 2
        assert np.array_equal(pts[i], cells[i]) and np.array_equal(vals[i], T.reconstruct(cells[i], means, b.bpv, q, 32768 >> 2)), f


@pytest.mark.gpu
def test_float32_device_frames_drop_and_index(batches):
    import torch
    b = batches("uint8")
    geo = b.geo
    rng = np.random.default_rng(12)
    voxel, origin = 0.05, (1.0, -2.0, 0.5)
    lats = [_cloud(rng, 3000), np.concatenate([b.frames[5][:2000], b.frames[5][:400]])]      # the second with duplicates
    attrs = [_colour(rng, 3000, 3, np.dtype(np.uint8)), _colour(rng, 2400, 2, np.dtype(np.uint16))]
    fl = [(p.astype(np.float32) * np.float32(voxel) + np.asarray(origin, np.float32)).astype(np.float32) for p in lats]
    want = geo.compress(lats, attributes=attrs, qstep=20, return_index=True)
    plain = geo.compress(lats, attributes=attrs, return_index=True)
    assert want[0] == plain[0] and all(np.array_equal(x, y) for x, y in zip(want[2], plain[2]))      # return_index is unchanged
    assert [x[1] for x in want[1]] == [19, 19]
    dev = geo.compress([torch.from_numpy(f).to(geo.rt.device) for f in fl], attributes=attrs, qstep=20, voxel=voxel, origin=origin,
                       return_index=True)
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
    hattrs = attrs + [np.zeros((5, 2), np.uint8)]
    ints = [p[v] for p, v in zip(lats, valid)] + [np.zeros((0, 3), np.int32)]      # the lattice points the kept rows came from
    kept = geo.compress(ints, attributes=[a[v] for a, v in zip(hattrs, valid)], qstep=20)      # the equivalent integer host call
    for frames in (holes, [torch.from_numpy(f).to(geo.rt.device) for f in holes]):
        drop = geo.compress(frames, attributes=hattrs, qstep=20, voxel=voxel, origin=origin, invalid="drop", return_index=True)
        assert drop[:2] == kept
        assert all(((np.asarray(i.cpu() if hasattr(i, "cpu") else i) >= 0) == v).all() for i, v in zip(drop[2], valid))
    assert kept[1][2] == bytes([ord("A"), 19, 1, 2]) + bytes(8)
    nothing = geo.compress([holes[2]], attributes=[hattrs[2]], qstep=20, voxel=voxel, origin=origin, invalid="drop")
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
             7: geo.compress(frames, attributes=attrs, scalable=True, max_error=2)[1],
             14: geo.compress(frames, attributes=attrs, scalable=True, max_error=2, cross_channel=True)[1],
             19: geo.compress(frames, attributes=attrs, qstep=9)[1]}
    alone = {k: geo.decompress(gb, ab)[1] for k, ab in kinds.items()}
    order = (19, 1, 7, 19, 14, 19, 19, 1)
    mix = [kinds[k][i] for i, k in enumerate(order)]
    assert [x[1] for x in mix] == list(order)
    for out in ("numpy", "device"):
        pts, vals = geo.decompress(gb, mix, output=out)
        for i, k in enumerate(order):
            p, v = (pts[i], vals[i]) if out == "numpy" else (pts[i].cpu().numpy(), vals[i].cpu().numpy())
            assert np.array_equal(p, b.pts[at[i]]) and np.array_equal(v, alone[k][i]), (out, i, k)
    # no levels of detail
    with pytest.raises(ValueError, match="frame 2: attributes of blob version 19"):
        geo.decompress(gb[:3], [kinds[7][0], kinds[7][1], kinds[19][2]], lod=1)
    with pytest.raises(abi.PccError) as e:
        G.attr_lod_info(kinds[19][0], 1)
    assert e.value.code == abi.PCC_E_ARG
    # another frame's geometry, with another point count
    with pytest.raises(abi.PccError) as e:
        geo.decompress([gb[0], gb[2]], [kinds[19][0], kinds[19][1]])
    assert e.value.code == abi.PCC_E_STREAM and "frame 1:" in str(e.value)
    # the entry points: the run kinds' refuses 19, the lod entry refuses it beside another kind and above lod 0
    with geo._lock, geo.rt as rt:
        cells = rt.octree_decode_frames(gb[:2], device=True, lod=0)
        for blobs_, kw in (([kinds[19][0]], {}), ([kinds[19][0], kinds[7][1]], {"lod": 0, "cells": cells}),
                           ([kinds[7][0], kinds[19][1]], {"lod": 0, "cells": cells}), ([kinds[19][0]], {"lod": 1, "cells": cells[:1]})):
            with pytest.raises(abi.PccError):
                rt.attr_decode_frames(blobs_, **kw)
    # damaged blobs are named, and the codec stays usable
    x = kinds[19][1]
    for what, bad in (("cut", x[:-2]), ("cut head", x[:15]), ("q = 0", x[:12] + bytes(4) + x[16:]), ("version 16", x[:1] + bytes([16]) + x[2:])):
        with pytest.raises(abi.PccError) as e:
            geo.decompress(gb[:3], [kinds[19][0], bad, kinds[19][2]])
        assert e.value.code == abi.PCC_E_STREAM and "frame 1:" in str(e.value), (what, str(e.value))
    assert all(np.array_equal(p, q) for p, q in zip(geo.decompress(gb, kinds[19])[1], alone[19]))


@pytest.mark.gpu
def test_a_recorded_frame_end_to_end(geo):
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        pts, colours = f["points_7"].astype(np.int32), f["colors_u8_7"]
    gb, lossless = geo.compress([pts], attributes=[colours])
    gb2, ab = geo.compress([pts], attributes=[colours], qstep=32)
    assert gb2 == gb
    dec, exact = geo.decompress(gb, lossless)
    lossy = geo.decompress(gb, ab)[1]
    want = T.reconstruct(dec[0], exact[0].astype(np.int64), 1, 32)
    assert ab[0] == T.encode(dec[0], exact[0].astype(np.int64), 1, 32) and np.array_equal(lossy[0], want)
    nl = geo.compress([pts], attributes=[colours], max_error=16)[1]
    assert len(ab[0]) < len(nl[0])
    rep = geo.distortion(dec, dec, attributes_a=exact, attributes_b=lossy)[0]
    mse = ((want - exact[0].astype(np.int64)) ** 2).sum(0) / want.shape[0]
    print(f"frame 7: {len(ab[0])} B against {len(nl[0])} B of max_error=16; mse per channel {rep['attr_mse_ab']}")
    assert rep["mse_ab"] == 0.0 and rep["attr_mse_ab"] == [float(m) for m in mse] == rep["attr_mse_ba"]


@pytest.mark.gpu
def test_the_default_calls_are_unchanged(batches):
    """qstep = 0 and no qstep: for one cloud each, the eight existing kinds give the bytes of their numpy restatements"""
    for dtype, f in (("uint8", 4), ("uint16", 3)):
        b = batches(dtype)
        pts, vals = b.pts[f], b.want[f]
        for scalable in (False, True):
            for e in (0, 2):
                for cross in (False, True):
                    want = attr_cross_ref.encode(vals, b.bpv, cross, e, points=pts if scalable else None) if cross else \
                        attr_nl_ref.encode(vals, b.bpv, e, points=pts if scalable else None)
                    kw = dict(scalable=scalable, max_error=e, cross_channel=cross)
                    assert b.geo.compress([b.frames[f]], attributes=[b.attrs[f]], **kw) == ([b.blobs[f]], [want]), (dtype, kw)
                    assert b.geo.compress([b.frames[f]], attributes=[b.attrs[f]], qstep=0, **kw)[1] == [want], (dtype, kw)
    assert attr_ref.encode(b.want[3], 2) == b.geo.compress([b.frames[3]], attributes=[b.attrs[3]])[1][0]
