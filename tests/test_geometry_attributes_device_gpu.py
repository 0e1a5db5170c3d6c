"""Device-resident and float attributes on the device (pcc_attr_stage_frames, GeometryCodec): device tensors are held
to the same values as host arrays byte for byte, float values to the restatement (tests/attr_stage_ref.py).
tests/test_geometry_attributes_device.py has the rule worked by hand.
"""
import ctypes as C

import numpy as np
import pytest

import attr_stage_ref as ref
import nn_ref
from conftest import pkg

pytestmark = pytest.mark.gpu

SIZES = [5, 0, 0, 1, 63, 64, 65, 257, 4000]      # two adjacent empty frames; 5 rows of 3 uint8 = 15 bytes in front of a pad


@pytest.fixture(scope="module")
def geo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg().GeometryCodec()
    yield g
    g.close()


@pytest.fixture(scope="module")
def room():
    """room(4000, seed=3), its points made distinct (int32 [n, 3], Morton order)"""
    fr = pkg("workloads").room(4000, seed=3)
    pts = nn_ref.morton_sorted_unique(fr["points"]).astype(np.int32)
    assert 3500 < pts.shape[0] <= 4000
    return pts


@pytest.fixture(scope="module")
def frames(room):
    """the room cut up into frames of SIZES rows (4000: all of it), each from another place"""
    out = []
    for f, n in enumerate(SIZES):
        n = min(n, room.shape[0])
        at = (97 * f) % (room.shape[0] - n + 1)
        out.append(np.ascontiguousarray(room[at:at + n]))
    return out


def dev(geo, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(geo.rt.device)


def values(frames, dtype, c, seed=1):
    """random values of `dtype`, [n, c] per frame; c == 0: 1-D"""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max + 1
    return [rng.integers(0, top, (p.shape[0],) + ((c,) if c else ())).astype(dtype) for p in frames]


def clean_call(geo):
    pts = np.array([[1, 2, 3], [4, 5, 6]], np.int32)
    a = np.array([[7, 8, 9], [10, 11, 12]], np.uint8)
    blobs, attr_blobs = geo.compress([pts], attributes=[dev(geo, a)])
    got_p, got_a = geo.decompress(blobs, attr_blobs)
    assert np.array_equal(got_p[0], pts) and np.array_equal(got_a[0], a)


# ------------------------------------------------------------------ device attributes against host attributes
@pytest.mark.parametrize("c", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_device_attributes_give_the_host_blobs(geo, frames, dtype, c):
    attrs = values(frames, dtype, c)
    want = geo.compress(frames, attributes=attrs)
    got = geo.compress(frames, attributes=[dev(geo, a) for a in attrs])
    assert got == want and len(want[1]) == len(SIZES)
    got = geo.compress([dev(geo, p) for p in frames], attributes=[dev(geo, a) for a in attrs])
    assert got == want


KINDS = [dict(), dict(scalable=True), dict(predictor="neighbours"), dict(max_error=2), dict(qstep=16, colour="ycocg"),
         dict(qstep=8, target_bytes=900), dict(cross_channel=True, lod=1)]


@pytest.mark.parametrize("kw", KINDS, ids=lambda kw: "-".join(kw) or "default")
def test_kinds(geo, frames, kw):
    attrs = values(frames, np.uint8, 3, seed=2)
    want = geo.compress(frames, attributes=attrs, **kw)
    d_attrs = [dev(geo, a) for a in attrs]
    assert geo.compress(frames, attributes=d_attrs, **kw) == want                          # host frames, device attributes
    assert geo.compress([dev(geo, p) for p in frames], attributes=d_attrs, **kw) == want   # both on the device
    mixed = [a if f % 2 else a.astype(np.uint16) << 3 for f, a in enumerate(attrs)]         # uint8 beside uint16 frames
    if "qstep" not in kw:
        assert geo.compress(frames, attributes=[dev(geo, a) for a in mixed], **kw) == geo.compress(frames, attributes=mixed, **kw)


def test_dropped_rows(geo, frames):
    xyz = [p.astype(np.float32) * 0.5 for p in frames[3:8]]
    for p in xyz[1:]:
        p[::7, 1] = np.nan
    xyz[2][-1] = np.inf
    attrs = values(xyz, np.uint16, 2, seed=3)
    kw = dict(voxel=0.5, invalid="drop", return_index=True)
    want = geo.compress(xyz, attributes=attrs, **kw)
    got = geo.compress(xyz, attributes=[dev(geo, a) for a in attrs], **kw)
    assert got[:2] == want[:2] and all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))
    assert any((i < 0).any() for i in want[2])
    # a call whose rows are all dropped, and a call without a row
    none = [np.full((4, 3), np.nan, np.float32)]
    a = [np.arange(8, dtype=np.uint8).reshape(4, 2)]
    assert geo.compress(none, attributes=[dev(geo, a[0])], voxel=1.0, invalid="drop") == \
        geo.compress(none, attributes=a, voxel=1.0, invalid="drop")
    empty = [np.zeros((0, 3), np.int32)] * 2
    a = [np.zeros((0, 3), np.uint8)] * 2
    assert geo.compress(empty, attributes=[dev(geo, x) for x in a]) == geo.compress(empty, attributes=a)


def test_strided_view_goes_in_by_pitch(geo, frames):
    import torch
    wide = [np.random.default_rng(4 + f).integers(0, 65536, (p.shape[0], 8)).astype(np.uint16) for f, p in enumerate(frames)]
    want = geo.compress(frames, attributes=[np.ascontiguousarray(w[:, 4:7]) for w in wide])
    views = [dev(geo, w)[:, 4:7] for w in wide]
    assert not views[-1].is_contiguous() and views[-1].stride() == (8, 1)
    assert geo.compress(frames, attributes=views) == want
    # a column (1-D, stride 8), and views that cannot go in by pitch: transposed, and one row broadcast
    cols = [dev(geo, w)[:, 5] for w in wide]
    assert cols[-1].stride() == (8,)
    assert geo.compress(frames, attributes=cols) == geo.compress(frames, attributes=[np.ascontiguousarray(w[:, 5]) for w in wide])
    t = [dev(geo, np.ascontiguousarray(w[:, 4:7].T)).T for w in wide]
    assert t[-1].stride(1) != 1
    assert geo.compress(frames, attributes=t) == want
    row = torch.tensor([[1, 2, 3]], dtype=torch.uint8, device=geo.rt.device)
    assert geo.compress(frames[-1:], attributes=[row.expand(frames[-1].shape[0], 3)]) == \
        geo.compress(frames[-1:], attributes=[np.tile(np.array([[1, 2, 3]], np.uint8), (frames[-1].shape[0], 1))])


# ------------------------------------------------------------------ float sources
def float_values(sizes, ft, s, c=3):
    """values in and around [0, peak / s], with exact ties, values below 0 and above the peak, -0.0 and a denormal"""
    rng = np.random.default_rng(11)
    peak = 255 if s <= 255 else 65535
    special = np.array([0.5, 1.5, 0.0625, 0.1875, -0.0, -3.7, 0.0, 1.0, 2.0 * peak / s, 1e30, -1e30,
                        np.finfo(ft).smallest_subnormal, (peak + 0.49) / s], ft)
    out = []
    for n in sizes:
        x = rng.uniform(-0.2, 1.2 * peak / s, (n, c)).astype(ft)
        x.reshape(-1)[:special.shape[0]] = special[:x.size]
        out.append(x)
    return out


@pytest.mark.parametrize("s", [255, 1000])
@pytest.mark.parametrize("ft", [np.float32, np.float64])
def test_float_sources(geo, frames, ft, s):
    fr = [frames[0], frames[1], frames[7], frames[5]]
    x = float_values([p.shape[0] for p in fr], ft, s)
    dtype = np.uint8 if s == 255 else np.uint16
    q = [ref.stage(a, s) for a in x]
    assert all(a.dtype == dtype for a in q)
    # the input holds what it is there for: exact ties (0.5 * 255 = 127.5; 0.0625 * 1000 = 62.5), both clamps
    prod = np.concatenate([a.reshape(-1) for a in x]).astype(np.float64) * s
    assert (np.abs(prod - np.floor(prod) - 0.5) == 0).any() and (prod < 0).any() and (prod > np.iinfo(dtype).max + 1).any()
    want = geo.compress(fr, attributes=q, return_index=True)
    host = geo.compress(fr, attributes=x, attribute_scale=s, return_index=True)
    device = geo.compress(fr, attributes=[dev(geo, a) for a in x], attribute_scale=s, return_index=True)
    assert host[:2] == want[:2] and device[:2] == want[:2]
    # decoded values are the restatement's (the frames are free of duplicates: nothing merges)
    _, dec = geo.decompress(device[0], device[1])
    for f in range(len(fr)):
        assert (dec[f].dtype == dtype or not q[f].size) and np.array_equal(dec[f][device[2][f]], q[f])
    # attribute_dtype: uint16 under s = 255 is cut at 65535 instead of 255, uint8 under s = 1000 at 255
    other = np.uint16 if s == 255 else np.uint8
    got = geo.compress(fr, attributes=[dev(geo, a) for a in x], attribute_scale=s, attribute_dtype=other)
    assert got == geo.compress(fr, attributes=[ref.stage(a, s, other) for a in x])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("ft", [np.float32, np.float64])
def test_non_finite_values_raise(geo, frames, ft, bad):
    abi = pkg("_abi")
    fr = [frames[0], frames[4]]
    x = float_values([p.shape[0] for p in fr], ft, 255)
    x[1][40, 2] = bad
    for attrs in (x, [dev(geo, a) for a in x]):
        with pytest.raises(abi.PccError, match="pcc_attr_stage_frames.*non-finite attribute") as e:
            geo.compress(fr, attributes=attrs, attribute_scale=255)
        assert e.value.code == abi.PCC_E_RANGE
        clean_call(geo)
    with pytest.raises(abi.PccError, match="non-finite attribute"):
        geo.transfer(fr, [dev(geo, a) for a in x], fr, attribute_scale=255)
    with pytest.raises(abi.PccError, match="non-finite attribute"):
        geo.distortion(fr, fr, [dev(geo, a) for a in x], [dev(geo, a) for a in x], attribute_scale=255)
    clean_call(geo)


def test_voxelized_frame_goes_straight_into_compress(geo):
    """capture.voxelize(output="device") -> compress(attribute_scale=255): points and float64 colours never leave the
    device, and the blobs are those of the host route through the restatement"""
    capture = pkg("capture")
    rng = np.random.default_rng(21)
    n = 3000
    xyz = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-1.2, -0.6, n)], 1)
    rgba = (rng.integers(0, 256, n, dtype=np.uint32) | (rng.integers(0, 256, n, dtype=np.uint32) << 8)
            | (rng.integers(0, 256, n, dtype=np.uint32) << 16) | (np.uint32(255) << 24))
    data = np.concatenate([xyz.astype(np.float32), rgba.view(np.float32)[:, None]], 1)
    rt = pkg("runtime").Runtime(0)      # the capture step's own runtime and stream
    try:
        with rt:
            host = capture.voxelize(rt, data, 1.4, 0.02)
            frame = capture.voxelize(rt, data, 1.4, 0.02, output="device")
            assert frame["colors"].is_cuda and str(frame["colors"].dtype) == "torch.float64" and frame["points"].is_cuda
            got = geo.compress([frame["points"]], attributes=[frame["colors"]], attribute_scale=255)
    finally:
        rt.close()
    assert 100 < host["points"].shape[0] < n and host["colors"].dtype == np.float64
    want = geo.compress([host["points"]], attributes=[ref.stage(host["colors"], 255)])
    assert got == want
    assert geo.compress([host["points"]], attributes=[host["colors"]], attribute_scale=255) == want


# ------------------------------------------------------------------ distortion, transfer, normals
def test_distortion_with_device_attributes(geo, room):
    a = [room[:257], room[300:1500], room[:0]]
    b = [p + np.array([1, 0, -1], np.int32) for p in a]
    b[1] = b[1][::2]
    rng = np.random.default_rng(5)
    va = [rng.integers(0, 256, (257, 3)).astype(np.uint8), rng.integers(0, 65536, (1200, 2)).astype(np.uint16), np.zeros((0, 4), np.uint8)]
    vb = [rng.integers(0, 256, (257, 3)).astype(np.uint8), rng.integers(0, 65536, (600, 2)).astype(np.uint16), np.zeros((0, 4), np.uint8)]
    want = geo.distortion(a, b, va, vb, peak=1023)
    assert want[1]["attr_mse_ab"][0] > 255 ** 2 and len(want[0]["attr_mse_ab"]) == 3      # a uint8 frame beside a uint16 frame
    d = lambda xs: [dev(geo, x) for x in xs]      # noqa: E731
    assert geo.distortion(a, b, d(va), d(vb), peak=1023) == want
    assert geo.distortion(d(a), d(b), d(va), d(vb), peak=1023) == want
    # float values on both sides, host and device, against the restatement's integers
    xa = [x.astype(np.float64) / 255.0 for x in (va[0], vb[0])]
    want = geo.distortion(a[:1], b[:1], [va[0]], [vb[0]])
    assert geo.distortion(a[:1], b[:1], [xa[0]], [xa[1]], attribute_scale=255) == want
    assert geo.distortion(a[:1], b[:1], d(xa[:1]), d(xa[1:]), attribute_scale=255) == want
    with pytest.raises(ValueError, match="attributes_a on the device, attributes_b on the host"):
        geo.distortion(a, b, d(va), vb)
    clean_call(geo)


def test_transfer_with_device_attributes(geo, room):
    import torch
    src = [room[:1000], room[1000:1257], room[:64]]
    src[0] = np.concatenate([src[0], src[0][:100]])      # duplicate rows merge
    dst = [np.ascontiguousarray(p[::3] + np.array([0, 1, 0], np.int32)) for p in src]
    rng = np.random.default_rng(6)
    v = [rng.integers(0, 256, (1100, 3)).astype(np.uint8), rng.integers(0, 65536, 257).astype(np.uint16),
         rng.integers(0, 256, (64, 4)).astype(np.uint8)]
    want, want_cnt = geo.transfer(src, v, dst, return_counts=True)
    got, cnt = geo.transfer(src, [dev(geo, x) for x in v], dst, output="device", return_counts=True)
    for g, w, gc, wc in zip(got, want, cnt, want_cnt):
        assert g.is_cuda and tuple(g.shape) == w.shape and str(g.dtype) == "torch." + w.dtype.name
        assert np.array_equal(g.cpu().numpy(), w) and np.array_equal(gc.cpu().numpy(), wc)
    # float values: the result is of the dtype they become
    x = [a.astype(np.float32) * np.float32(0.25) for a in v]
    want = geo.transfer(src, [ref.stage(a, 4, np.uint16).reshape(a.shape) for a in x], dst)
    got = geo.transfer(src, [dev(geo, a) for a in x], dst, attribute_scale=4, attribute_dtype=np.uint16)
    assert all(g.dtype == np.uint16 and np.array_equal(g, w) for g, w in zip(got, want)) and got[1].ndim == 1
    # the chain of DESIGN.md 6c-transfer with no host array in between
    d_src, d_dst = [dev(geo, p) for p in src[:1]], [dev(geo, p) for p in dst[:1]]
    moved = geo.transfer(d_src, [dev(geo, v[0])], d_dst, output="device")
    blobs, attr_blobs = geo.compress(d_dst, attributes=moved, max_error=3)
    pts, lossy = geo.decompress(blobs, attr_blobs, output="device")
    rep = geo.distortion(pts, pts, attributes_a=geo.transfer(d_dst, moved, pts, output="device"), attributes_b=lossy)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in moved + pts + lossy)
    h_moved = geo.transfer(src[:1], v[:1], dst[:1])
    h_pts, h_lossy = geo.decompress(*geo.compress(dst[:1], attributes=h_moved, max_error=3))
    assert rep == geo.distortion(h_pts, h_pts, attributes_a=geo.transfer(dst[:1], h_moved, h_pts), attributes_b=h_lossy)
    assert rep[0]["mse_ab"] == 0.0 and 0 < max(rep[0]["attr_mse_ab"]) <= 9.0


def planes(seed):
    """three 20 x 20 lattice patches far from each other, in the planes z = 7, x = 300 and y = -200, rows shuffled: the
    k <= 16 nearest neighbours of a point lie in its own plane, so its normal is a unit vector of an axis, exactly"""
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2)
    z = np.zeros((400, 1), np.int64)
    pts = np.concatenate([np.concatenate([g, z + 7], 1), np.concatenate([z + 300, g - 100], 1),
                          np.concatenate([g[:, :1] - 300, z - 200, g[:, 1:] + 150], 1)]).astype(np.int32)
    return pts[np.random.default_rng(seed).permutation(pts.shape[0])]


def test_device_normals_feed_distortion(geo, room):
    """normals(output="device") -> distortion(normals_a=...).  pcc_nn_d2_frames adds a frame's projections in an
    unspecified order (include/pcc.h), so two runs over the same normals agree to the last bit only where the sum is
    exact: on the planes every normal is a unit vector of an axis and every projection an integer, and there every
    figure of the device route equals the host route's.  On the room the d2 figures are held to the bound of a float64
    sum of n non-negative terms in any order, n 2^-52 relative, and every other figure to equality."""
    import torch
    a = [planes(1), planes(2)[:900]]
    b = [np.ascontiguousarray(p[::2] + np.array([1, 2, 3], np.int32)) for p in a]
    normals = geo.normals(a, k=12)
    d_normals = geo.normals(a, k=12, output="device")
    assert all(t.is_cuda and np.array_equal(t.cpu().numpy(), n) for t, n in zip(d_normals, normals))
    for n in normals:      # the input holds the case: axis normals, all three axes
        assert np.array_equal(np.unique(np.abs(n), axis=0), np.eye(3, dtype=np.float32)[::-1])
    want = geo.distortion(a, b, normals_a=normals, peak=1023)
    assert all(r["d2_mse_ab"] > 1 and r["d2_mse_ab"] != r["mse_ab"] and r["d2_mse_ba"] > 1 for r in want)
    for fa, fb in ((a, b), ([dev(geo, p) for p in a], [dev(geo, p) for p in b])):
        assert geo.distortion(fa, fb, normals_a=d_normals, peak=1023) == want
    # normals that are not of an axis: shuffled rows would show in the d2 figures, the order of the sum within the bound
    ra = [room[:500], room[500:1700]]
    rb = [np.ascontiguousarray(p[::2] + np.array([1, 1, 0], np.int32)) for p in ra]
    r_normals = geo.normals(ra, k=12)
    r_want = geo.distortion(ra, rb, normals_a=r_normals, peak=1023)
    r_got = geo.distortion(ra, rb, normals_a=geo.normals(ra, k=12, output="device"), peak=1023)
    for g, w, pa in zip(r_got, r_want, ra):
        assert {k: v for k, v in g.items() if not k.startswith("d2_")} == {k: v for k, v in w.items() if not k.startswith("d2_")}
        for key in ("d2_mse_ab", "d2_mse_ba"):
            print(key, g[key], w[key])
            assert w[key] > 0 and abs(g[key] - w[key]) <= 2 * (pa.shape[0] + 1) * 2.0 ** -52 * max(g[key], w[key])
    normals, d_normals = r_normals, geo.normals(ra, k=12, output="device")
    a, b, want = ra, rb, r_want
    bad = [d_normals[0], d_normals[1].clone()]
    bad[1][77, 1] = float("nan")
    with pytest.raises(ValueError, match="^frame 1: non-finite normal"):
        geo.distortion(a, b, normals_a=bad)
    with pytest.raises(ValueError, match="frame 1: normals on the host, frame 0's on the device"):
        geo.distortion(a, b, normals_a=[d_normals[0], normals[1]])
    with pytest.raises(TypeError, match="frame 0: expected float32 normals"):
        geo.distortion(a, b, normals_a=[t.to(torch.float64) for t in d_normals])
    assert geo.distortion(a, b, normals_a=d_normals, peak=1023)[0]["mse_ab"] == want[0]["mse_ab"]      # a clean call


def test_a_tensor_written_on_a_side_stream_just_before_the_call(geo, frames):
    import torch
    p = frames[-1]
    a = values([p], np.uint8, 3, seed=9)[0]
    want = geo.compress([p], attributes=[a])
    src = dev(geo, a)
    t = torch.zeros_like(src)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=geo.rt.device)
    with torch.cuda.stream(side):
        big = torch.empty(1 << 30, dtype=torch.uint8, device=geo.rt.device)
        for _ in range(12):      # a few milliseconds of work in front of the write
            big.fill_(1)
        t.copy_(src)
        got = geo.compress([p], attributes=[t])
    assert got == want
    side.synchronize()


# ------------------------------------------------------------------ refusals, each followed by a clean call
def test_refusals(geo, frames):
    import torch
    p = frames[4:6]
    u8 = values(p, np.uint8, 3)
    cases = [
        (ValueError, "frame 1: attributes on the host, frame 0's on the device", dict(attributes=[dev(geo, u8[0]), u8[1]])),
        (ValueError, "frame 1: attributes on the device, frame 0's on the host", dict(attributes=[u8[0], dev(geo, u8[1])])),
        (TypeError, "frame 0: expected uint8 or uint16 attributes, got float16", dict(attributes=[dev(geo, a).to(torch.float16) for a in u8])),
        (TypeError, "frame 0: expected uint8 or uint16 attributes, got int32", dict(attributes=[dev(geo, a).to(torch.int32) for a in u8])),
        (TypeError, "frame 0: expected uint8 or uint16 attributes, got float32.*attribute_scale",
         dict(attributes=[dev(geo, a).to(torch.float32) for a in u8])),
        (TypeError, "frame 0: expected uint8 or uint16 attributes, got float64.*attribute_scale", dict(attributes=[a / 255.0 for a in u8])),
        (ValueError, "frame 0: attribute_scale with uint8 attributes", dict(attributes=[dev(geo, a) for a in u8], attribute_scale=255)),
        (ValueError, "attribute_scale quantises float attributes: it needs attributes", dict(attribute_scale=255)),
    ]
    x = [dev(geo, a / 255.0) for a in u8]
    for s in (0, 70000, float("nan")):
        cases.append((ValueError, "0 < s <= 65535", dict(attributes=x, attribute_scale=s)))
    cases.append((ValueError, "attribute_dtype must be np.uint8 or np.uint16", dict(attributes=x, attribute_scale=255, attribute_dtype=np.int8)))
    cases.append((ValueError, "attribute_dtype is what float attributes become", dict(attributes=u8, attribute_dtype=np.uint8)))
    for err, text, kw in cases:
        with pytest.raises(err, match=text):
            geo.compress(p, **kw)
        clean_call(geo)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="frame 0: attributes on cuda:1"):
            geo.compress(p, attributes=[torch.from_numpy(a).to("cuda:1") for a in u8])
        clean_call(geo)


# ------------------------------------------------------------------ the C-ABI, called directly
REC = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("out", "<i8"), ("kind", "<i4"), ("c", "<i4")])


def stage_direct(geo, sources, s, bpv, channels, perm, tail=64):
    """pcc_attr_stage_frames on arrays of the test's own: sources (host array [n, c], pitch) go up as they are with
    `pitch` elements per row; the output is 0xEE everywhere before the call and `tail` bytes longer than it needs to be.
    -> (output bytes, value offsets, status)"""
    import torch
    rt = geo.rt
    nf = len(sources)
    offs = np.cumsum([0] + [a.shape[0] for a, _ in sources]).astype(np.int64)
    table = np.zeros(nf, REC)
    keep, at = [], 0
    for f, (a, pitch) in enumerate(sources):
        wide = np.full((a.shape[0], pitch), 77, a.dtype)
        wide[:, :a.shape[1]] = a
        d = dev(geo, wide)
        keep.append(d)
        own = a.dtype.itemsize if a.dtype.kind == "u" else bpv
        table[f] = (d.data_ptr() if a.shape[0] else 0, pitch, at, ref.KINDS[a.dtype], a.shape[1])
        at += (a.shape[0] * a.shape[1] * own + 15) // 16 * 16
    n = int(offs[-1])
    need = n * channels * bpv if channels else at
    with rt:
        out = torch.full((need + tail,), 0xEE, dtype=torch.uint8, device=rt.device)
        d_table, d_offs = dev(geo, table.view(np.uint8)), dev(geo, offs)
        d_perm = None if perm is None else dev(geo, np.asarray(perm, np.uint32).view(np.int32))
        status = torch.zeros(1, dtype=torch.int32, device=rt.device)
        code = rt.lib.pcc_attr_stage_frames(rt.ctx, C.c_void_p(table.ctypes.data), C.c_void_p(d_table.data_ptr()),
                                            C.c_void_p(offs.ctypes.data), C.c_void_p(d_offs.data_ptr()), nf, float(s), bpv, channels,
                                            None if d_perm is None else C.c_void_p(d_perm.data_ptr()), C.c_void_p(out.data_ptr()),
                                            need, C.c_void_p(status.data_ptr()))
        assert code == 0, rt.lib.pcc_last_error()
        rt.sync()
        return out.cpu().numpy(), table["out"].tolist(), int(status.item())


def direct_sources(seed=31):
    rng = np.random.default_rng(seed)
    x32 = float_values([65], np.float32, 255, c=2)[0]
    x64 = float_values([257], np.float64, 255, c=4)[0]
    return [(rng.integers(0, 256, (5, 3)).astype(np.uint8), 3), (np.zeros((0, 2), np.uint16), 2),
            (rng.integers(0, 256, (63, 1)).astype(np.uint8), 4), (x32, 2), (rng.integers(0, 65536, (64, 3)).astype(np.uint16), 7),
            (x64, 5), (rng.integers(0, 256, (1, 4)).astype(np.uint8), 4), (rng.integers(0, 65536, (700, 1)).astype(np.uint16), 1)]


@pytest.mark.parametrize("bpv", [1, 2])
def test_cabi_packed(geo, bpv):
    sources = direct_sources()
    dtype = np.uint8 if bpv == 1 else np.uint16
    want, offs = ref.packed([a for a, _ in sources], 255, dtype)
    got, got_offs, status = stage_direct(geo, sources, 255, bpv, 0, None)
    assert got_offs == offs and status == 0
    assert (want == 0xEE).sum() > 20      # pads between the frames: the kernel leaves them alone
    assert np.array_equal(got[:want.shape[0]], want) and (got[want.shape[0]:] == 0xEE).all()


@pytest.mark.parametrize("bpv, channels", [(1, 4), (2, 2), (2, 4)])
def test_cabi_sorted(geo, bpv, channels):
    sources = [(a, p) for a, p in direct_sources() if a.shape[1] <= channels and (bpv == 2 or a.dtype != np.uint16)]
    assert len(sources) >= 4
    dtype = np.uint8 if bpv == 1 else np.uint16
    n = sum(a.shape[0] for a, _ in sources)
    perm = np.random.default_rng(2).permutation(n).astype(np.int64)
    want = ref.sorted_rows([a for a, _ in sources], perm, dtype, channels, 255)
    got, _, status = stage_direct(geo, sources, 255, bpv, channels, perm)
    assert status == 0
    assert np.array_equal(got[:want.nbytes].view(dtype).reshape(n, channels), want) and (got[want.nbytes:] == 0xEE).all()
    # entries outside the call: zero rows and status bit 1, nothing else disturbed
    perm[[0, 70, n - 1]] = [n, 2 ** 32 - 1, n + 5]
    want = ref.sorted_rows([a for a, _ in sources], perm, dtype, channels, 255)
    got, _, status = stage_direct(geo, sources, 255, bpv, channels, perm)
    assert status == 2 and not want[[0, 70, n - 1]].any()
    assert np.array_equal(got[:want.nbytes].view(dtype).reshape(n, channels), want) and (got[want.nbytes:] == 0xEE).all()


def test_cabi_non_finite_sets_bit_0(geo):
    x = np.array([[0.5, np.nan]], np.float32)
    _, _, status = stage_direct(geo, [(x, 2)], 255, 1, 0, None)
    assert status == 1
    _, _, status = stage_direct(geo, [(np.array([[np.inf, 1.0]]), 2)], 255, 2, 2, [0])
    assert status == 1


def test_cabi_refusals_leave_the_context_usable(geo):
    import torch
    abi = pkg("_abi")
    rt = geo.rt
    fn = rt.lib.pcc_attr_stage_frames
    src = dev(geo, np.arange(24, dtype=np.float32).reshape(8, 3))
    u8 = dev(geo, np.arange(24, dtype=np.uint8).reshape(8, 3))
    out = torch.zeros(256, dtype=torch.uint8, device=rt.device)
    status = torch.zeros(1, dtype=torch.int32, device=rt.device)
    perm = dev(geo, np.arange(8, dtype=np.int32))

    def call(kind=2, c=3, pitch=3, rows=(0, 8), nf=1, s=255.0, bpv=1, channels=0, use_perm=False, null=None, out_off=0, ptr=None,
             out_bytes=256):
        table = np.zeros(max(nf, 1), REC)
        table[0] = ((src if kind >= 2 else u8).data_ptr() if ptr is None else ptr, pitch, out_off, kind, c)
        offs = np.array(list(rows) + [rows[-1]] * max(nf - 1, 0), np.int64)
        d_table, d_offs = dev(geo, table.view(np.uint8)), dev(geo, offs)
        args = [C.c_void_p(table.ctypes.data), C.c_void_p(d_table.data_ptr()), C.c_void_p(offs.ctypes.data), C.c_void_p(d_offs.data_ptr()),
                nf, s, bpv, channels, C.c_void_p(perm.data_ptr()) if use_perm else None, C.c_void_p(out.data_ptr()), out_bytes,
                C.c_void_p(status.data_ptr())]
        if null is not None:
            args[null] = None
        with rt:
            return fn(rt.ctx, *args)

    assert call() == 0 and call(channels=4, use_perm=True) == 0 and call(kind=0, s=float("nan")) == 0      # integers read no scale
    bad = [dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=11), dict(null=9), dict(nf=0), dict(nf=65536),
           dict(rows=(0, 1 << 27)), dict(rows=(0, -1)), dict(rows=(1, 8)), dict(kind=4), dict(kind=-1), dict(c=0), dict(c=5),
           dict(pitch=2), dict(s=0.0), dict(s=-1.0), dict(s=float("nan")), dict(s=float("inf")), dict(bpv=3), dict(channels=3),
           dict(channels=2, use_perm=True), dict(bpv=2, channels=2, use_perm=True), dict(channels=4), dict(use_perm=True),
           dict(out_off=8), dict(out_bytes=23), dict(ptr=src.data_ptr() + 2), dict(kind=1, bpv=1, channels=4, use_perm=True)]
    for kw in bad:
        assert call(**kw) == abi.PCC_E_ARG, kw
        assert b"pcc_attr_stage_frames" in rt.lib.pcc_last_error(), kw
    assert int(status.item()) == 0 and call() == 0
    rt.sync()
    assert out.cpu().numpy()[:24].tolist() == ref.quantise(np.arange(24, dtype=np.float32), 255, np.uint8).tolist()
    clean_call(geo)
