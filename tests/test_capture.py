"""GPU voxelisation of a camera frame (capturer.py:88-126) against the numpy
restatement in oracle/capture_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import capture_cases as cases
from capture_cases import GRID
from conftest import pkg


def camera_frame(seed, w=160, h=120, far=False):
    """ZED-like XYZRGBA float32 [w*h,4]: a wall, a sphere and a floor seen from the origin, with NaN /
    inf pixels and some points beyond the depth clip"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(-0.6, 0.6, w), np.linspace(-0.45, 0.45, h))
    d = np.stack([u, v, -np.ones_like(u)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = np.full(d.shape[0], 1.2)                                    # back wall at z = -1.2
    t = np.where(d[:, 1] < -0.05, np.minimum(t, -0.35 / np.minimum(d[:, 1], -1e-6)), t)   # floor y = -0.35
    c = np.array([0.1, 0.0, -0.8])
    b = d @ c
    disc = b * b - (c @ c - 0.2 ** 2)
    ts = np.where(disc > 0, b - np.sqrt(np.maximum(disc, 0)), np.inf)
    t = np.where((ts > 0) & (ts < t), ts, t)
    p = (d * t[:, None] + rng.normal(0, 0.0008, d.shape)).astype(np.float32)
    if far:
        p[::17] *= 3.0                                              # beyond depth_clip
    p[::101] = np.nan
    p[5::211, 0] = np.inf
    rgba = (rng.integers(0, 256, d.shape[0], dtype=np.uint32) | (rng.integers(0, 256, d.shape[0], dtype=np.uint32) << 8)
            | (rng.integers(0, 256, d.shape[0], dtype=np.uint32) << 16) | (np.uint32(255) << 24))
    return np.concatenate([p, rgba.view(np.float32)[:, None]], 1).astype(np.float32)


def test_oracle_matches_dictionary_form():
    """the sorted-segment restatement and the one-accumulator-per-voxel form agree"""
    from oracle import capture_ref as ref
    data = camera_frame(1, 80, 60, far=True)
    out = ref.voxelize(data, 1.4, 0.01)
    d = ref.voxelize_open3d_semantics(data, 1.4, 0.01)
    pts = [tuple(int(v) for v in p) for p in out["points"]]
    assert sorted(pts) == sorted(d.keys()) and pts == sorted(pts)
    for p, col in zip(pts, out["colors"]):
        assert any(np.array_equal(np.asarray(c), col) for c in d[p])
    assert out["colors"].min() >= 0 and out["colors"].max() <= 1
    capped = ref.voxelize(data, 1.4, 0.01, max_points=500)
    assert capped["points"].shape[0] == 500
    assert capped["points"][:, 2].min() >= np.sort(out["points"][:, 2])[-500]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,voxel,max_points,far", [(1, 0.005, None, True), (2, 0.01, 3000, False),
                                                        (3, 0.02, None, True), (4, 0.005, 30000, True)])
def test_voxelize_gpu_equals_oracle(rt, seed, voxel, max_points, far):
    from oracle import capture_ref as ref
    capture = pkg("capture")
    data = camera_frame(seed, far=far)
    out = capture.voxelize(rt, data, 1.4, voxel, max_points)
    exp = ref.voxelize(data, 1.4, voxel, max_points)
    assert out["points"].dtype == np.int16 and out["colors"].dtype == np.float64
    assert np.array_equal(out["points"], exp["points"])
    assert np.array_equal(out["colors"], exp["colors"])
    assert np.unique(out["points"], axis=0).shape[0] == out["points"].shape[0]


@pytest.mark.gpu
def test_voxelize_edge_cases(rt):
    capture = pkg("capture")
    assert capture.voxelize(rt, np.zeros((0, 4), np.float32))["points"].shape == (0, 3)
    allnan = np.full((50, 4), np.nan, np.float32)
    assert capture.voxelize(rt, allnan)["points"].shape == (0, 3)
    one = np.array([[0.1, -0.2, -0.5, 0.0]], np.float32)
    one[0, 3] = np.array([0x00FF8040], np.uint32).view(np.float32)[0]
    out = capture.voxelize(rt, one, 1.4, 0.005)
    assert out["points"].tolist() == [[20, -40, -100]]
    assert np.allclose(out["colors"], [[0x40 / 255, 0x80 / 255, 0xFF / 255]], rtol=0, atol=0)


@pytest.mark.gpu
def test_voxelized_frame_goes_through_the_codec(rt):
    """capture pre-step -> compress -> decompress, the chain of the demo's sender and receiver"""
    capture = pkg("capture")
    wl = pkg("workloads")
    frame = capture.voxelize(rt, camera_frame(7), 1.4, 0.005, 30000)
    enc = pkg("codec_pipeline").CompressionPipeline([[1, 1]], slots=1)
    dec = pkg("codec_parallel").DecompressionPipeline(slots=1)
    out, side = enc.compress(wl.gop([frame]))
    rec, _ = dec.decompress(out[1])
    assert rec[0]["points"].shape[0] == frame["points"].shape[0]


# ---------------------------------------------------------------------------------------------------------
# The edges a camera frame reaches: rows beyond pcc_vox_valid's capped grid, minima of either sign, norms at
# the depth clip, rint ties, dense voxels, duplicates after rounding, the max_points edges, device in / out,
# the two refusals.  Inputs: tests/capture_cases.py.  Every non-emptiness condition is asserted on the CPU.


@functools.lru_cache(maxsize=None)
def _expected(case, *args):
    """restatement's answer for a cached input, computed once: ('name', generator args..., clip, voxel, max_points)"""
    from oracle import capture_ref as ref
    *gen, clip, voxel, max_points = args
    data = getattr(cases, case)(*gen)
    return ref.voxelize(data[0] if isinstance(data, tuple) else data, clip, voxel, max_points)


def _same(out, exp):
    assert out["points"].dtype == np.int16 and out["colors"].dtype == np.float64
    assert np.array_equal(out["points"], exp["points"])
    assert np.array_equal(out["colors"].view(np.uint64), exp["colors"].view(np.uint64))     # to the last bit


def _rows(out):
    return [tuple(int(v) for v in p) for p in out["points"]]


def test_ties_and_merge_by_hand():
    """voxel 0.5, depth clip 100; point i (i = 0..7): x = -1.25 + 0.5 i, y = 2.25 - 0.5 i, z = 0.25, colour
    (10 i + 1, 10 i + 2, 10 i + 3).  Every value and quotient is exact in binary.

    min_bound = (-1.25, -1.25, 0.25), voxel_min_bound = min_bound - 0.25 = (-1.5, -1.5, 0):
    Open3D index of point i = floor((x + 1.5) / 0.5, (y + 1.5) / 0.5, 0.25 / 0.5) = (i, 7 - i, 0) — eight voxels of
    one point each, in x-major index order 0..7, mean = the point.
    x / 0.5 = -2.5 -1.5 -0.5 0.5 1.5 2.5 3.5 4.5  -> half-to-even  -2 -2 -0 0 2 2 4 4
    y / 0.5 =  4.5  3.5  2.5 1.5 0.5 -0.5 -1.5 -2.5 ->              4  4  2 2 0 -0 -2 -2
    z / 0.5 =  0.5                                  ->              0
    Points (0,1), (2,3), (4,5), (6,7) merge: rows [-2,4,0] [0,2,0] [2,0,0] [4,-2,0], each with the colour of the
    smaller Open3D index, i.e. of input points 0, 2, 4, 6.  Round-half-away would give x = -3 -2 -1 1 2 3 4 5:
    eight distinct rows."""
    from oracle import capture_ref as ref
    data = cases.ties_frame()
    assert np.array_equal(data[:, :3].astype(np.float64) / 0.5 % 1.0, np.full((8, 3), 0.5))    # all 24 on a tie
    out = ref.voxelize(data, cases.TIES_CLIP, cases.TIES_VOXEL)
    assert out["points"].tolist() == [[-2, 4, 0], [0, 2, 0], [2, 0, 0], [4, -2, 0]]
    rgb = np.array([[10 * i + 1, 10 * i + 2, 10 * i + 3] for i in (0, 2, 4, 6)], np.float64)
    assert np.array_equal(out["colors"], rgb / 255.0)
    away = cases.round_half_away(data[:, :3].astype(np.float64) / 0.5)
    assert away[:, 0].tolist() == [-3, -2, -1, 1, 2, 3, 4, 5]
    assert np.unique(away, axis=0).shape[0] == 8
    d = ref.voxelize_open3d_semantics(data, cases.TIES_CLIP, cases.TIES_VOXEL)
    assert sorted(d) == _rows(out) and all(len(c) == 2 for c in d.values())


def _lattice_ties(data):
    """quotients mean / voxel of the lattice cloud that sit exactly on .5, as (negative, positive) counts"""
    q = cases.voxel_means(data, cases.TIES_CLIP, cases.TIES_VOXEL) / cases.TIES_VOXEL
    tie = q - np.floor(q) == 0.5
    return int((tie & (q < 0)).sum()), int((tie & (q > 0)).sum()), q


def test_lattice_cloud_has_ties_of_both_signs():
    """on the quarter lattice the restatement's integer voxels are rint (half-to-even) of exact means; ties of
    both signs occur and round-half-away would give other rows"""
    data = cases.lattice_cloud()
    neg, pos, q = _lattice_ties(data)
    assert neg > 0 and pos > 0
    exp = _expected("lattice_cloud", cases.TIES_CLIP, cases.TIES_VOXEL, None)
    even = np.unique(np.rint(q).astype(np.int64), axis=0)
    away = np.unique(cases.round_half_away(q).astype(np.int64), axis=0)
    assert np.array_equal(exp["points"], even.astype(np.int16))
    assert not np.array_equal(even, away)
    assert data[:, :3].min() < 0 < data[:, :3].max()


def _check_against_dictionary(data, clip, voxel, out):
    from oracle import capture_ref as ref
    d = ref.voxelize_open3d_semantics(data, clip, voxel)
    pts = _rows(out)
    assert sorted(pts) == sorted(d.keys()) and pts == sorted(pts)
    for p, col in zip(pts, out["colors"]):
        assert any(np.array_equal(np.asarray(c), col) for c in d[p])
    return d


def test_oracle_matches_dictionary_form_dense_and_duplicates():
    """the dictionary form on the dense-voxel input (one candidate per voxel: colours equal to the last bit)
    and on the duplicate input (several Open3D voxels per integer voxel: the kept colour is one of theirs)"""
    data = cases.dense_cloud(20000)
    out = _expected("dense_cloud", 20000, cases.CLIP, cases.DENSE_VOXEL, None)
    d = _check_against_dictionary(data, cases.CLIP, cases.DENSE_VOXEL, out)
    assert len(d) == 27 and all(len(c) == 1 for c in d.values())
    data = cases.collision_cloud()
    out = _expected("collision_cloud", cases.CLIP, cases.COLLISION_VOXEL, None)
    d = _check_against_dictionary(data, cases.CLIP, cases.COLLISION_VOXEL, out)
    assert sum(len(set(c)) > 1 for c in d.values()) >= 1          # the smallest-index rule decides something


def _assert_clip_classes(data, cls):
    """rows exactly on the clip, one ulp either side, and rows a double-precision norm would put elsewhere"""
    clip = np.float32(cases.CLIP)
    n32, n64 = cases.norm32(data), cases.norm64(data)
    assert np.array_equal(n32[cls == 0], np.full((cls == 0).sum(), clip))
    assert np.array_equal(n32[cls == -1], np.full((cls == -1).sum(), np.nextafter(clip, np.float32(0))))
    assert np.array_equal(n32[cls == 1], np.full((cls == 1).sum(), np.nextafter(clip, np.float32(2))))
    assert all((cls == c).sum() > 0 for c in (-1, 0, 1)) and np.isin(cls, (-1, 0, 1)).all()
    inside = n32 <= clip
    assert ((n64 <= np.float64(clip)) != inside).sum() > 0                      # double, compared unrounded
    assert ((n64.astype(np.float32) <= clip) != inside).sum() > 0               # double, rounded at the end
    return inside


def test_depth_clip_in_the_restatement():
    """valid = finite and sqrt((x*x + y*y) + z*z) <= float32(clip), every step rounded to float32: rows exactly
    on the clip stay, rows one ulp beyond go, whatever a double-precision norm says"""
    from oracle import capture_ref as ref
    data, cls = cases.clip_rows()
    inside = _assert_clip_classes(data, cls)
    assert np.array_equal(inside, cls <= 0)
    assert np.array_equal(ref.valid_mask(data, cases.CLIP), inside)
    assert np.array_equal(np.linalg.norm(data[:, :3], axis=1), cases.norm32(data))
    assert ref.voxelize(data, cases.CLIP, 0.01)["points"].shape[0] == \
        ref.voxelize(data[inside], cases.CLIP, 0.01)["points"].shape[0] > 0


def _vox_valid(rt, data, clip):
    """pcc_vox_valid through the C-ABI: (valid bytes, min bound float32 [3], n_valid)"""
    import torch
    m = data.shape[0]
    d = rt.to_device(data, torch.float32)
    valid = torch.full((m,), 7, dtype=torch.uint8, device=rt.device)
    mn = (C.c_float * 3)(9.0, 9.0, 9.0)
    nv = C.c_int64(-1)
    rc = rt.lib.pcc_vox_valid(rt.ctx, C.c_void_p(d.data_ptr()), m, C.c_float(float(np.float32(clip))),
                              C.c_void_p(valid.data_ptr()), mn, C.byref(nv))
    assert rc == 0, rt.lib.pcc_last_error()
    return valid.cpu().numpy(), np.array(list(mn), np.float32), nv.value


STRIDED_M = [1, 255, 256, 257, GRID - 1, GRID, GRID + 1, GRID + 300, 2 * GRID + 1]


def _strided_mask(m, variant):
    """the frame, the restatement's mask, and the CPU-side check of where the minima sit"""
    from oracle import capture_ref as ref
    data = cases.strided_frame(m, variant)
    mask = ref.valid_mask(data, cases.CLIP)
    assert mask.any() and (m == 1 or not mask.all())
    mn = data[mask, :3].min(axis=0)
    if m > GRID:
        assert mask[:GRID].sum() >= 2000 and mask[GRID:].sum() >= 1
        for a in range(3):
            holders = np.flatnonzero(mask & (data[:, a] == mn[a]))
            assert holders.min() >= (2 * GRID if m == 2 * GRID + 1 and not (variant == "zero" and a == 0) else GRID)
    sign = {"positive": (1, 1, 1), "negative": (-1, -1, -1), "mixed": (1, -1, -1), "zero": (0, 1, -1)}[variant]
    assert np.sign(mn).tolist() == list(sign)
    if variant == "zero" and m >= GRID + 300:
        zeros = data[mask & (data[:, 0] == 0), 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    return data, mask, mn


@pytest.mark.gpu
@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("m", STRIDED_M)
def test_vox_valid_strided_and_signs(rt, m, variant):
    """pcc_vox_valid alone: mask, per-axis minimum and count of frames up to two full strides of its capped
    grid plus one row, with the minima in rows only the strided loop reaches, for minima of either sign"""
    data, mask, mn = _strided_mask(m, variant)
    valid, got_mn, nv = _vox_valid(rt, data, cases.CLIP)
    assert nv == int(mask.sum())
    assert np.array_equal(valid, mask.astype(np.uint8))
    assert np.array_equal(got_mn, mn)           # by value: the sign of a zero minimum does not reach the result


@pytest.mark.gpu
@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("m", [GRID + 300, 2 * GRID + 1])
def test_voxelize_strided_frames(rt, m, variant):
    capture = pkg("capture")
    data, mask, _ = _strided_mask(m, variant)
    exp = _expected("strided_frame", m, variant, cases.CLIP, 0.01, None)
    n = exp["points"].shape[0]
    assert n > 1000
    _same(capture.voxelize(rt, data, cases.CLIP, 0.01), exp)
    _same(capture.voxelize(rt, data, cases.CLIP, 0.01, n // 3), _expected("strided_frame", m, variant, cases.CLIP, 0.01, n // 3))


@pytest.mark.gpu
def test_depth_clip_gpu(rt):
    """norms exactly on the clip and one ulp either side: the float32 step-by-step rule with <=, not a fused,
    reordered or double-precision norm, and not <"""
    from oracle import capture_ref as ref
    capture = pkg("capture")
    data, cls = cases.clip_rows()
    inside = _assert_clip_classes(data, cls)
    valid, mn, nv = _vox_valid(rt, data, cases.CLIP)
    assert np.array_equal(valid, ref.valid_mask(data, cases.CLIP).astype(np.uint8))
    assert np.array_equal(valid.astype(bool), inside) and nv == int(inside.sum())
    assert np.array_equal(mn, data[inside, :3].min(axis=0))
    _same(capture.voxelize(rt, data, cases.CLIP, 0.01), _expected("clip_rows", cases.CLIP, 0.01, None))


@pytest.mark.gpu
def test_ties_by_hand_gpu(rt):
    """the frame of test_ties_and_merge_by_hand: half-to-even, four merged rows, colours of points 0, 2, 4, 6"""
    capture = pkg("capture")
    data = cases.ties_frame()
    out = capture.voxelize(rt, data, cases.TIES_CLIP, cases.TIES_VOXEL)
    assert out["points"].tolist() == [[-2, 4, 0], [0, 2, 0], [2, 0, 0], [4, -2, 0]]
    rgb = np.array([[10 * i + 1, 10 * i + 2, 10 * i + 3] for i in (0, 2, 4, 6)], np.float64)
    assert np.array_equal(out["colors"], rgb / 255.0)
    from oracle import capture_ref as ref
    _same(out, ref.voxelize(data, cases.TIES_CLIP, cases.TIES_VOXEL))


@pytest.mark.gpu
def test_lattice_ties_gpu(rt):
    """quarter lattice at voxel 0.5: voxel boundaries on points, means exactly on .5, both signs"""
    capture = pkg("capture")
    data = cases.lattice_cloud()
    neg, pos, _ = _lattice_ties(data)
    assert neg > 0 and pos > 0
    _same(capture.voxelize(rt, data, cases.TIES_CLIP, cases.TIES_VOXEL),
          _expected("lattice_cloud", cases.TIES_CLIP, cases.TIES_VOXEL, None))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 70000])
def test_dense_voxels_gpu(rt, n):
    """27 voxels of n / 27 points: the double sums depend on the order, which is the input order (stable sort,
    single-workgroup at 20000 keys and multi-kernel at 70000, then k_vox_mean's run loop)"""
    from oracle import capture_ref as ref
    capture = pkg("capture")
    data = cases.dense_cloud(n)
    exp = _expected("dense_cloud", n, cases.CLIP, cases.DENSE_VOXEL, None)
    rev = ref.voxelize(data[::-1], cases.CLIP, cases.DENSE_VOXEL)
    assert exp["points"].shape[0] == 27 and np.array_equal(rev["points"], exp["points"])
    assert not np.array_equal(rev["colors"], exp["colors"])          # the case can see a wrong order
    _same(capture.voxelize(rt, data, cases.CLIP, cases.DENSE_VOXEL), exp)


@pytest.mark.gpu
def test_duplicates_after_rounding_gpu(rt):
    """several Open3D voxels round to one integer voxel: the one with the smallest Open3D index is kept"""
    from oracle import capture_ref as ref
    capture = pkg("capture")
    data = cases.collision_cloud()
    d = ref.voxelize_open3d_semantics(data, cases.CLIP, cases.COLLISION_VOXEL)
    assert sum(len(set(c)) > 1 for c in d.values()) >= 1
    _same(capture.voxelize(rt, data, cases.CLIP, cases.COLLISION_VOXEL),
          _expected("collision_cloud", cases.CLIP, cases.COLLISION_VOXEL, None))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["0", "1", "n-1", "n", "n+1"])
def test_max_points_edges_gpu(rt, which):
    """the cap around the uncapped voxel count n, on a frame whose z takes 17 values (ties at every threshold)"""
    capture = pkg("capture")
    data = cases.lattice_cloud()
    full = _expected("lattice_cloud", cases.TIES_CLIP, cases.TIES_VOXEL, None)
    n = full["points"].shape[0]
    assert n > 20 * np.unique(full["points"][:, 2]).shape[0]
    k = {"0": 0, "1": 1, "n-1": n - 1, "n": n, "n+1": n + 1}[which]
    exp = _expected("lattice_cloud", cases.TIES_CLIP, cases.TIES_VOXEL, k)
    assert exp["points"].shape[0] == min(k, n)
    _same(capture.voxelize(rt, data, cases.TIES_CLIP, cases.TIES_VOXEL, k), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("max_points", [None, 700])
def test_device_input_and_output_gpu(rt, max_points):
    import torch
    capture = pkg("capture")
    data = cases.collision_cloud()
    host = capture.voxelize(rt, data, cases.CLIP, cases.COLLISION_VOXEL, max_points)
    _same(host, _expected("collision_cloud", cases.CLIP, cases.COLLISION_VOXEL, max_points))
    dev_in = torch.from_numpy(data).to(rt.device)
    _same(capture.voxelize(rt, dev_in, cases.CLIP, cases.COLLISION_VOXEL, max_points), host)
    out = capture.voxelize(rt, dev_in, cases.CLIP, cases.COLLISION_VOXEL, max_points, output="device")
    assert out["points"].is_cuda and out["points"].dtype == torch.int32 and out["points"].shape[1] == 3
    assert out["colors"].is_cuda and out["colors"].dtype == torch.float64
    assert np.array_equal(out["points"].cpu().numpy(), host["points"].astype(np.int32))
    assert np.array_equal(out["colors"].cpu().numpy().view(np.uint64), host["colors"].view(np.uint64))
    assert np.array_equal(dev_in.cpu().numpy().view(np.uint32), data.view(np.uint32))       # input left alone


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,extent,word", [(1e-7, 0.5, "2^21"), (2e-5, 0.8, "outside int16")])
def test_refusals_gpu(rt, voxel, extent, word):
    """finite frames the step must refuse: more than 2^21 Open3D voxels per axis; integer voxels beyond int16
    (the restatement wraps there, like the reference's astype(int16)).  The runtime stays usable."""
    capture = pkg("capture")
    abi = pkg("_abi")
    rng = np.random.default_rng(21)
    data = cases.pack(rng.uniform(-extent, extent, (2000, 3)), rng)
    span = float((data[:, :3].max(axis=0) - data[:, :3].min(axis=0)).max()) / voxel
    assert cases.norm32(data).max() < cases.CLIP and np.abs(data[:, :3]).max() / voxel > 32768
    assert span > 2 ** 21 if word == "2^21" else span < 2 ** 20
    with pytest.raises(abi.PccError) as e:
        capture.voxelize(rt, data, cases.CLIP, voxel)
    assert e.value.code == abi.PCC_E_RANGE and word in str(e.value)
    _same(capture.voxelize(rt, cases.collision_cloud(), cases.CLIP, cases.COLLISION_VOXEL),
          _expected("collision_cloud", cases.CLIP, cases.COLLISION_VOXEL, None))
