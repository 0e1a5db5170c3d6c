"""Metric frames of GeometryCodec: float32 and device-resident frames in (pcc_morton_keys_frames_f32), rows without a
return dropped, the row index out (pcc_rows_index), float32 points back (pcc_points_to_metric).  The rule is the one of
include/pcc.h, restated in tests/metric_ref.py; every blob must equal, byte for byte, the blob of the restatement's
lattice points coded as int32 frames."""
import os

import numpy as np
import pytest

import metric_ref
from conftest import ROOT, pkg, random_cloud

GRIDS = [(0.02, (0.0, 0.0, 0.0)), (0.25, (-16.0, 8.5, 2.0))]      # 0.02 is not a float32; 0.25 makes exact halves


def test_metric_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    for name in ("pcc_morton_keys_frames_f32", "pcc_rows_index", "pcc_points_to_metric"):
        assert name + "(" in text
        assert name in abi.PROTOTYPES


# ------------------------------------------------------------------ the restatement, on the CPU
def _col(xs, o=0.0):
    """rows (x, o, o) of float32"""
    p = np.full((len(xs), 3), o, np.float32)
    p[:, 0] = np.asarray(xs, np.float32)
    return p


def test_restatement_worked_by_hand():
    # halves round to even
    lat, valid, status = metric_ref.quantize(_col([0.5, 1.5, 2.5, -0.5, -1.5, 3.49, -2.51]), 1.0)
    assert lat[:, 0].tolist() == [0, 2, 2, 0, -2, 3, -3] and valid.all() and status == 0
    # ... with a voxel and an origin that keep the halves exact: (x - 3) / 0.25
    lat, valid, status = metric_ref.quantize(_col([3.125, 3.375, 3.625, 2.875], 3.0), 0.25, (3.0, 3.0, 3.0))
    assert lat.tolist() == [[0, 0, 0], [2, 0, 0], [2, 0, 0], [0, 0, 0]] and status == 0
    # the range edges are accepted, one step beyond each is flagged; a half below the upper edge's next step rounds in
    lat, valid, status = metric_ref.quantize(_col([-32768.0, 32767.0, 32767.49, -32768.5]), 1.0)
    assert lat[:, 0].tolist() == [-32768, 32767, 32767, -32768] and status == 0
    for beyond in (32768.0, -32769.0, 32767.5, 1e30, -3e38):
        lat, valid, status = metric_ref.quantize(_col([1.0, beyond]), 1.0)
        assert status == metric_ref.OFF_GRID and valid.all() and lat[1].tolist() == [0, 0, 0], beyond
    # edges under a non-zero origin: q = (x - 100) / 0.5
    lat, valid, status = metric_ref.quantize(_col([100 - 16384.0, 100 + 16383.5], 100.0), 0.5, (100.0, 100.0, 100.0))
    assert lat[:, 0].tolist() == [-32768, 32767] and status == 0
    assert metric_ref.quantize(_col([100 + 16384.0], 100.0), 0.5, (100.0, 100.0, 100.0))[2] == metric_ref.OFF_GRID
    # NaN, +Inf, -Inf rows are not valid, in whichever coordinate
    p = _col([1.0, np.nan, np.inf, -np.inf, 2.0])
    p[4, 2] = np.nan
    lat, valid, status = metric_ref.quantize(p, 1.0)
    assert valid.tolist() == [True, False, False, False, False] and status == metric_ref.NON_FINITE
    assert lat[0].tolist() == [1, 0, 0] and not lat[1:].any()
    p[0, 1] = 40000.0
    assert metric_ref.quantize(p, 1.0)[2] == metric_ref.OFF_GRID | metric_ref.NON_FINITE
    # backwards: lattice points, and cell centres at k = 1, 2, 15 with the most negative cell
    assert metric_ref.dequantize([[0, 1, -1]], 0, 0.25, (1.0, 2.0, 3.0)).tolist() == [[1.0, 2.25, 2.75]]
    assert metric_ref.centres([[-16384, 0, 16383]], 1).tolist() == [[-32767.5, 0.5, 32766.5]]
    assert metric_ref.centres([[-8192, 0, 8191]], 2).tolist() == [[-32766.5, 1.5, 32765.5]]
    assert metric_ref.centres([[-1, 0, 0]], 15).tolist() == [[-16384.5, 16383.5, 16383.5]]
    assert metric_ref.dequantize([[-16384, 0, 16383]], 1, 2.0, (1.0, 1.0, 1.0)).tolist() == [[-65534.0, 2.0, 65534.0]]
    assert metric_ref.dequantize([[-1, 0, 0]], 15, 0.5, (0.25, 0.0, 0.0)).tolist() == [[-8192.0, 8191.75, 8191.75]]


def test_cell_centres_are_exact_in_float32():
    for k in range(16):
        c = np.arange(-32768 >> k, (32767 >> k) + 1)
        t = metric_ref.centres(c, k)
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t), k
        assert t[0] == -32768 + ((1 << k) - 1) / 2 and t[-1] == 32767 - ((1 << k) - 1) / 2


@pytest.mark.parametrize("voxel,origin", [(0.02, (0, 0, 0)), (0.02, (12.5, -3.25, 1.73)), (0.001, (0.1, 0.2, 0.3)),
                                          (0.05, (-400, 250, 10)), (1.0, (0, 0, 0)), (0.0123, (7, 7, 7))])
def test_round_trip_bound(voxel, origin):
    """|dequantize(quantize(x)) - x| <= v / 2 + 2^-21 (|x| + |o| + v) per coordinate: half a cell, and six float32
    roundings (x - o, / v, the integer's conversion is exact, t * v, o + .; v and o themselves count) of relative size
    2^-24 on magnitudes no larger than |x| + |o| + v: 6 * 2^-24 < 2^-21"""
    rng = np.random.default_rng(20261)
    v, o = np.float32(voxel), np.asarray(origin, np.float32)
    u = rng.uniform(-32760.0, 32760.0, (2_000_000, 3))
    x = (o.astype(np.float64) + u * float(v)).astype(np.float32)
    lat, valid, status = metric_ref.quantize(x, voxel, origin)
    assert status == 0 and valid.all()
    back = metric_ref.dequantize(lat, 0, voxel, origin).astype(np.float64)
    x64 = x.astype(np.float64)
    err = np.abs(back - x64)
    bound = float(v) / 2 + 2.0 ** -21 * (np.abs(x64) + np.abs(o.astype(np.float64)) + float(v))
    assert (err <= bound).all(), float((err - bound).max())


# ------------------------------------------------------------------ GPU
def _metres(pts, voxel, origin, rng, jitter=0.45):
    """integer points taken back to the caller's unit and moved off the lattice, float32"""
    p = np.asarray(pts, np.float64)
    x = np.asarray(origin, np.float64) + (p + rng.uniform(-jitter, jitter, p.shape)) * float(np.float32(voxel))
    return x.astype(np.float32)


def _hand(voxel, origin):
    """halves (exact ones under the second grid) and the range edges"""
    v, o = float(np.float32(voxel)), np.asarray(origin, np.float64)
    t = np.array([[0.5, 1.5, 2.5], [-0.5, -1.5, -2.5], [3.5, 4.5, -7.5], [100.5, -100.5, 0.5], [0.5, 0.5, 0.5],
                  [1.5, 1.5, 1.5], [32767, 32767, 32767], [-32768, -32768, -32768], [32767, -32768, 0.5],
                  [-32768, 5, 9], [0, 0, 0], [32766.5, -32767.5, 2.5]], np.float64)
    return (o + t * v).astype(np.float32)


def _frames(wl, voxel, origin, with_room=True):
    rng = np.random.default_rng(77)
    ints = [wl.lidar_sweep(seed=1)["points"], wl.lidar_sweep(seed=2)["points"]]
    if with_room:
        ints.append(wl.room(1_000_000, seed=0)["points"])
    frames = [_metres(p, voxel, origin, rng) for p in ints]
    frames += [_hand(voxel, origin), np.zeros((0, 3), np.float32), _metres([[5, -6, 7]], voxel, origin, rng),
               _metres([[1, 2, 3], [-4, 5, -6]], voxel, origin, rng)]
    return frames


def _lattice(frames, voxel, origin):
    out = []
    for f in frames:
        lat, valid, status = metric_ref.quantize(f, voxel, origin)
        assert status == 0 and valid.all()
        out.append(lat)
    return out


def _attrs(frames, rng):
    out = []
    for i, f in enumerate(frames):
        n = f.shape[0]
        out.append(rng.integers(0, 65536, (n, 2)).astype(np.uint16) if i % 2 else rng.integers(0, 256, n).astype(np.uint8))
    return out


@pytest.fixture(scope="module")
def geo():
    g = pkg().GeometryCodec()
    yield g
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,origin", GRIDS)
def test_float_frames_code_the_restatements_lattice(geo, oracle, wl, voxel, origin):
    frames = _frames(wl, voxel, origin)
    lat = _lattice(frames, voxel, origin)
    hand = lat[3]
    if voxel == 0.25:      # the exact halves went to the even neighbour
        assert hand[0].tolist() == [0, 2, 2] and hand[1].tolist() == [0, -2, -2] and hand[-1].tolist() == [32766, -32768, 2]
    assert hand[6].tolist() == [32767] * 3 and hand[7].tolist() == [-32768] * 3
    blobs = geo.compress(frames, voxel=voxel, origin=origin)
    want = geo.compress(lat)
    assert len(blobs) == len(frames)
    for f, (b, w) in enumerate(zip(blobs, want)):
        assert b == w, f"frame {f}: blob differs from the lattice points' ({len(b)} vs {len(w)} bytes)"
    for f in (0, 1):
        assert blobs[f] == oracle.octree_encode(np.unique(lat[f], axis=0), 32768, version=2), f
    assert len(blobs[4]) == 24
    assert geo.compress(frames, lod=2, voxel=voxel, origin=origin) == geo.compress(lat, lod=2)
    attrs = _attrs(frames, np.random.default_rng(5))
    for kw in ({}, {"scalable": True}, {"scalable": True, "lod": 2}):
        got = geo.compress(frames, attributes=attrs, voxel=voxel, origin=origin, **kw)
        ref = geo.compress(lat, attributes=attrs, **kw)
        assert got[0] == ref[0] and got[0] == (want if "lod" not in kw else geo.compress(lat, lod=2)), kw
        assert got[1] == ref[1], kw


@pytest.mark.gpu
def test_device_frames_give_the_host_frames_bytes(geo, wl):
    import torch
    voxel, origin = GRIDS[1]
    frames = _frames(wl, voxel, origin, with_room=False)
    lat = _lattice(frames, voxel, origin)
    attrs = _attrs(frames, np.random.default_rng(6))
    want = geo.compress(frames, attributes=attrs, voxel=voxel, origin=origin)
    dev = [torch.from_numpy(f).to(geo.rt.device) for f in frames]
    assert geo.compress(dev, attributes=attrs, voxel=voxel, origin=origin) == want
    assert geo.compress(dev, voxel=voxel, origin=origin, lod=2) == geo.compress(lat, lod=2)
    host_t = [torch.from_numpy(f) for f in frames]
    assert geo.compress(host_t, voxel=voxel, origin=origin) == want[0]
    # integer frames on the device, int16 and int32 and both in one call
    for dtypes in ((np.int16,), (np.int32,), (np.int16, np.int32)):
        ints = [l.astype(dtypes[i % len(dtypes)]) for i, l in enumerate(lat)]
        got = geo.compress([torch.from_numpy(a).to(geo.rt.device) for a in ints], attributes=attrs)
        assert got[0] == want[0] and got[1] == want[1], dtypes
        assert geo.compress([torch.from_numpy(a) for a in ints]) == want[0], dtypes


@pytest.mark.gpu
def test_frame_and_grid_errors(geo):
    import torch
    d = geo.rt.device
    f32 = np.zeros((4, 3), np.float32)
    i32 = np.zeros((4, 3), np.int32)
    with pytest.raises(ValueError, match="frame 1"):      # host beside device
        geo.compress([torch.zeros(4, 3, device=d), f32], voxel=1.0)
    with pytest.raises(ValueError, match="frame 2"):      # a host tensor beside device tensors
        geo.compress([torch.zeros(4, 3, device=d), torch.zeros(4, 3, device=d), torch.zeros(4, 3)], voxel=1.0)
    with pytest.raises(ValueError, match="frame 1"):      # integer beside float
        geo.compress([f32, i32], voxel=1.0)
    with pytest.raises(ValueError, match="frame 1"):
        geo.compress([torch.zeros(4, 3, dtype=torch.int32, device=d), torch.zeros(4, 3, device=d)])
    with pytest.raises(TypeError, match="float64"):
        geo.compress([np.zeros((4, 3), np.float64)], voxel=1.0)
    with pytest.raises(TypeError, match="float64"):
        geo.compress([torch.zeros(4, 3, dtype=torch.float64, device=d)], voxel=1.0)
    with pytest.raises(ValueError, match="voxel"):      # integer frames are on the lattice already
        geo.compress([i32], voxel=0.02)
    with pytest.raises(ValueError, match="voxel"):      # float frames need it
        geo.compress([f32])
    for bad in (0.0, -0.02, float("nan"), float("inf"), 1e-50):      # 1e-50 is 0 as float32
        with pytest.raises(ValueError, match="voxel"):
            geo.compress([f32], voxel=bad)
        with pytest.raises(ValueError, match="voxel"):
            geo.decompress([], voxel=bad)
    for bad in ((0.0, 1.0), (0.0, float("nan"), 0.0), (0.0, 0.0, 1e39)):
        with pytest.raises(ValueError, match="origin"):
            geo.compress([f32], voxel=1.0, origin=bad)
    with pytest.raises(ValueError, match="invalid"):
        geo.compress([f32], voxel=1.0, invalid="ignore")
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="frame 0"):
            geo.compress([torch.zeros(4, 3, device="cuda:1")], voxel=1.0)
    assert geo.compress([i32], invalid="drop") == geo.compress([i32])      # accepted, no effect


def _holes(frames, rng, share=0.05):
    """a seeded share of every frame's rows loses one coordinate to NaN, +Inf or -Inf"""
    out, valid = [], []
    for f in frames:
        f = f.copy()
        n = f.shape[0]
        rows = rng.permutation(n)[:int(round(share * n))]
        f[rows, rng.integers(0, 3, rows.size)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), rows.size)
        out.append(f)
        valid.append(np.isfinite(f).all(axis=1))
    return out, valid


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_invalid_rows_raise_or_drop(geo, wl, device):
    import torch
    abi = pkg("_abi")
    voxel, origin = GRIDS[0]
    rng = np.random.default_rng(404)
    clean = _frames(wl, voxel, origin, with_room=False)
    frames, valid = _holes(clean, rng)
    frames.append(np.full((7, 3), np.nan, np.float32))      # a frame without a single return
    valid.append(np.zeros(7, bool))
    assert sum(int((~v).sum()) for v in valid) > 5000
    attrs = _attrs(frames, np.random.default_rng(7))
    put = (lambda fs: [torch.from_numpy(f).to(geo.rt.device) for f in fs]) if device else (lambda fs: fs)
    with pytest.raises(abi.PccError) as e:
        geo.compress(put(frames), voxel=voxel, origin=origin)
    assert e.value.code == abi.PCC_E_RANGE and "non-finite" in str(e.value)
    kept = [f[v] for f, v in zip(frames, valid)]
    want = geo.compress(kept, attributes=[a[v] for a, v in zip(attrs, valid)], voxel=voxel, origin=origin)  # still usable
    assert want[0][:-1] == geo.compress(clean_kept(clean, valid), voxel=voxel, origin=origin)
    got = geo.compress(put(frames), attributes=attrs, voxel=voxel, origin=origin, invalid="drop")
    assert got[0] == want[0] and got[1] == want[1]
    assert len(got[0][-1]) == 24 and len(got[0][3]) == 24      # the frame of NaN rows, and the empty one
    assert geo.compress(put(frames), voxel=voxel, origin=origin, invalid="drop", lod=2) == \
        geo.compress(kept, voxel=voxel, origin=origin, lod=2)
    for kw in ({"scalable": True}, {"scalable": True, "lod": 2}):
        a = geo.compress(put(frames), attributes=attrs, voxel=voxel, origin=origin, invalid="drop", **kw)
        b = geo.compress(kept, attributes=[x[v] for x, v in zip(attrs, valid)], voxel=voxel, origin=origin, **kw)
        assert a[0] == b[0] and a[1] == b[1], kw
    # NaN rows only, alone in a call
    only = geo.compress(put([frames[-1]]), attributes=[attrs[-1]], voxel=voxel, origin=origin, invalid="drop")
    assert len(only[0][0]) == 24 and only[1] == [want[1][-1]]
    # a finite row off the grid is a wrong grid, not a missing return: it raises under both settings
    off = frames[0].copy()
    off[11] = [0.0, 32768 * voxel, 0.0]
    for mode in ("raise", "drop"):
        with pytest.raises(abi.PccError) as e:
            geo.compress(put([frames[1], off]), voxel=voxel, origin=origin, invalid=mode)
        assert e.value.code == abi.PCC_E_RANGE, mode
        assert ("non-finite" in str(e.value)) == (mode == "raise"), (mode, str(e.value))
    off = clean[0].copy()
    off[11] = [0.0, -3e38, 0.0]
    with pytest.raises(abi.PccError) as e:
        geo.compress(put([off]), voxel=voxel, origin=origin)
    assert e.value.code == abi.PCC_E_RANGE and "off the grid" in str(e.value)
    assert geo.compress(put(kept), voxel=voxel, origin=origin) == want[0]      # and the codec stays usable


def clean_kept(clean, valid):
    """the kept rows taken from the frames before the holes were made: the holes changed nothing else"""
    return [f[v] for f, v in zip(clean, valid)]


def _dup_frame(rng):
    dup = random_cloud(rng, 3000, extent=200, lo=-100)[:, 1:]
    return np.concatenate([dup, dup[:700], dup[::5]], 0)[rng.permutation(3000 + 700 + 600)]


def _check_index(geo, frames_in, lats, valids, blobs, index, lod, device):
    dec = geo.decompress(blobs)
    assert len(index) == len(frames_in)
    for f, (lat, valid, d, ix) in enumerate(zip(lats, valids, dec, index)):
        if device:
            assert ix.is_cuda
            ix = ix.cpu().numpy()
        assert isinstance(ix, np.ndarray) and ix.dtype == np.int32 and ix.shape == (lat.shape[0],), f
        assert (ix[~valid] == -1).all(), f
        assert np.array_equal(d[ix[valid]], lat[valid] >> lod), f
        assert np.array_equal(np.unique(ix[valid]), np.arange(d.shape[0])), f


@pytest.mark.gpu
@pytest.mark.parametrize("lod", [0, 2])
@pytest.mark.parametrize("device", [False, True])
def test_index_properties(geo, wl, lod, device):
    import torch
    voxel, origin = GRIDS[1]
    rng = np.random.default_rng(12 + lod)
    sweep = wl.lidar_sweep(seed=1)["points"]
    base = [_metres(sweep, voxel, origin, rng), _metres(_dup_frame(rng), voxel, origin, rng, jitter=0.0),
            np.zeros((0, 3), np.float32), _hand(voxel, origin), _metres([[5, -6, 7]], voxel, origin, rng)]
    put = (lambda fs: [torch.from_numpy(np.ascontiguousarray(f)).to(geo.rt.device) for f in fs]) if device else (lambda fs: fs)
    # float frames, nothing dropped
    q = [metric_ref.quantize(f, voxel, origin) for f in base]
    lats, valids = [x[0] for x in q], [x[1] for x in q]
    blobs, index = geo.compress(put(base), lod=lod, voxel=voxel, origin=origin, return_index=True)
    assert blobs == geo.compress(lats, lod=lod)
    _check_index(geo, base, lats, valids, blobs, index, lod, device)
    # the same as integer frames
    blobs_i, index_i = geo.compress(put(lats), lod=lod, return_index=True)
    assert blobs_i == blobs
    _check_index(geo, lats, lats, valids, blobs_i, index_i, lod, device)
    # with dropped rows, a frame that loses all of them, and attributes
    holes, valids = _holes(base, rng, share=0.1)
    holes.append(np.full((3, 3), np.inf, np.float32))
    valids.append(np.zeros(3, bool))
    lats = [metric_ref.quantize(f, voxel, origin)[0] for f in holes]
    attrs = _attrs(holes, np.random.default_rng(8))
    blobs, attr_blobs, index = geo.compress(put(holes), attributes=attrs, lod=lod, voxel=voxel, origin=origin,
                                            invalid="drop", return_index=True)
    _check_index(geo, holes, lats, valids, blobs, index, lod, device)
    dec, dec_attrs = geo.decompress(blobs, attr_blobs)
    for f, (a, ix, got) in enumerate(zip(attrs, index, dec_attrs)):
        ix = ix.cpu().numpy() if device else ix
        a = (a[:, None] if a.ndim == 1 else a).astype(np.int64)
        m = dec[f].shape[0]
        total, cnt = np.zeros((m, a.shape[1]), np.int64), np.zeros(m, np.int64)
        np.add.at(total, ix[ix >= 0], a[ix >= 0])
        np.add.at(cnt, ix[ix >= 0], 1)
        assert (cnt > 0).all() and got.dtype == attrs[f].dtype
        assert np.array_equal(got, (total + cnt[:, None] // 2) // cnt[:, None]), f
    # every row dropped, and no frame at all
    blobs, index = geo.compress(put([holes[-1]]), voxel=voxel, origin=origin, invalid="drop", return_index=True)
    assert len(blobs[0]) == 24 and (index[0].cpu().numpy() if device else index[0]).tolist() == [-1, -1, -1]
    assert geo.compress([], return_index=True) == ([], [])
    assert geo.compress([], attributes=[], return_index=True) == ([], [], [])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,origin", GRIDS)
def test_metric_points_out(geo, wl, voxel, origin):
    GeometryCodec = pkg().GeometryCodec
    frames = _frames(wl, voxel, origin, with_room=False)
    attrs = _attrs(frames, np.random.default_rng(9))
    blobs, attr_blobs = geo.compress(frames, attributes=attrs, scalable=True, voxel=voxel, origin=origin)
    for lod in (0, 2):
        cut = [b[:GeometryCodec.lod_info(b, lod)[0]] for b in blobs]
        acut = [a[:GeometryCodec.attr_lod_info(a, lod)[0]] for a in attr_blobs]
        cells = geo.decompress(cut, lod=lod)
        want = [metric_ref.dequantize(c, lod, voxel, origin) for c in cells]
        got = geo.decompress(cut, lod=lod, voxel=voxel, origin=origin)
        dev = geo.decompress(cut, output="device", lod=lod, voxel=voxel, origin=origin)
        for f, (w, g, d) in enumerate(zip(want, got, dev)):
            assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == w.shape, (lod, f)
            assert np.array_equal(_bits(g), _bits(w)), (lod, f)
            assert d.is_cuda and d.dtype.is_floating_point and np.array_equal(_bits(d.cpu().numpy()), _bits(w)), (lod, f)
        # together with version-2 attribute blobs: the same points, the attributes unchanged
        _, ref_attrs = geo.decompress(cut, acut, lod=lod)
        for output in ("numpy", "device"):
            pts, got_attrs = geo.decompress(cut, acut, output=output, lod=lod, voxel=voxel, origin=origin)
            for f, (w, p, a, r) in enumerate(zip(want, pts, got_attrs, ref_attrs)):
                if output == "device":
                    p, a = p.cpu().numpy(), a.cpu().numpy()
                assert np.array_equal(_bits(p), _bits(w)), (lod, output, f)
                assert a.dtype == r.dtype and np.array_equal(a, r), (lod, output, f)
    # version-1 attribute blobs at lod 0
    blobs1, attr1 = geo.compress(frames, attributes=attrs, voxel=voxel, origin=origin)
    pts, a1 = geo.decompress(blobs1, attr1, voxel=voxel, origin=origin)
    _, r1 = geo.decompress(blobs1, attr1)
    assert all(np.array_equal(_bits(p), _bits(metric_ref.dequantize(c, 0, voxel, origin)))
               for p, c in zip(pts, geo.decompress(blobs1)))
    assert all(np.array_equal(a, r) for a, r in zip(a1, r1))
    assert geo.decompress([], voxel=voxel, origin=origin) == []
