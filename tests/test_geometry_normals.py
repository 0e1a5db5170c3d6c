"""GeometryCodec.normals, the D2 figures of GeometryCodec.distortion, pcc_knn_frames and pcc_nn_d2_frames (include/pcc.h
has the rules, tests/normals_ref.py restates them by brute force).  Rows, distances and scatter matrices are integers
and held to equality; a normal is held to the Rayleigh check: it lies in the eigenspace of the smallest eigenvalue.

CPU: the restatement worked by hand, the ABI, the traversal replayed on the host (pcc_knn_replay_host is the kernel's
search and epilogue compiled for the host), the refusals that need no device.
GPU: the kernels against the restatement on the smallest shapes at which they can go wrong.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import nn_ref
import normals_ref
from conftest import ROOT, pkg, surface_cloud

KS = (3, 8, 16, 32)


# ------------------------------------------------------------------ shared cases (host arrays, computed once)
def _cloud(rng, n, lo, hi):
    """n distinct points of [lo, hi)^3"""
    pts = np.unique(rng.integers(lo, hi, (4 * n, 3)), axis=0)
    return pts[rng.permutation(pts.shape[0])[:n]]


def _frame_sizes():
    """frames of 3, k - 1, k, k + 1 (every k of KS), 64, 65, 257 and 2 999 points, an empty frame between two others,
    and the 257-point frame twice: nothing may leak across a frame in key order"""
    rng = np.random.default_rng(31)
    sizes = [3, 2, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 0, 257, 2999]
    frames = [_cloud(rng, n, -60, 60) for n in sizes]
    return frames + [frames[-2].copy()]


def _ties():
    """a full 8 x 8 x 8 block, and the seams of the distortion tests: neighbours in space far apart in key order"""
    g = np.arange(8)
    frames = [np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) - 4]
    for s in (0, 2, -2, 16, -16, 256, -256):
        frames.append(np.array([[s - 1] * 3, [s] * 3, [s - 1, s, s - 1], [s - 2, s - 1, s - 1], [s + 1, s, s], [s - 1, s - 1, s - 3],
                                [s, s + 2, s], [s - 3, s - 3, s - 3], [s + 2, s + 2, s + 2]]))
    return frames


def _range_and_pruning():
    """the two far corners in one frame (differences reach 65535, squared sums exceed 2^32), a tight cluster with one
    far outlier (large cells are skipped, the list fills late), a surface"""
    rng = np.random.default_rng(32)
    corners = np.concatenate([_cloud(rng, 50, -32768, -32760), _cloud(rng, 50, 32760, 32768)])
    outlier = np.concatenate([_cloud(rng, 300, 100, 112), [[20000, -15000, 9000]]])
    return [corners, outlier, surface_cloud(rng, 1500)[:, 1:]]


def _flat():
    """a lattice plane z = 5 (x, y on a 6 x 6 grid of spacing 4) and a line of 40 points"""
    g = 4 * np.arange(6)
    plane = np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2), np.full((36, 1), 5)], 1)
    return [plane, np.stack([np.arange(40), 2 * np.arange(40), -np.arange(40)], 1)]


CASES = {"frame sizes": _frame_sizes, "ties": _ties, "range and pruning": _range_and_pruning, "flat": _flat}


class Case:
    """the frames of one call in Morton order, their keys, and the brute-force neighbours at k = 32, of which every
    smaller k is a prefix"""

    def __init__(self, frames):
        self.frames = [nn_ref.morton_sorted_unique(f) for f in frames]
        self.keys = np.concatenate([nn_ref.morton_keys(f, i) for i, f in enumerate(self.frames)])
        assert np.all(np.diff(self.keys.astype(object)) > 0)
        self.knn32 = [normals_ref.knn(f, 32) for f in self.frames]
        self.points = np.concatenate(self.frames)
        self.has_normal = np.concatenate([np.full(f.shape[0], f.shape[0] >= 3) for f in self.frames])

    def expected(self, k):
        """(rows [n, k] counted over the call, d2 [n, k], C [n, 6])"""
        rows, d2s, cs, first = [], [], [], 0
        for p, (r, d) in zip(self.frames, self.knn32):
            r, d = r[:, :k], d[:, :k]
            cs.append(normals_ref.scatter(p, r))
            rows.append(np.where(r >= 0, r + first, -1))
            d2s.append(d)
            first += p.shape[0]
        return np.concatenate(rows), np.concatenate(d2s), np.concatenate(cs)


@pytest.fixture(scope="module")
def cases():
    return {name: Case(make()) for name, make in CASES.items()}


def _check_normals(case, cov, normals):
    """the Rayleigh check for every point that has a normal, zeros for the others"""
    has = case.has_normal
    assert normals.dtype == np.float32 and normals.shape == (has.shape[0], 3)
    assert normals_ref.rayleigh_check(cov[has], normals[has]) == 0
    assert not normals[~has].any() and not cov[~has].any()


# ------------------------------------------------------------------ CPU
def test_knn_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    for name in ("pcc_knn_frames", "pcc_nn_d2_frames", "pcc_knn_replay_host"):
        assert name + "(" in text
        assert name in abi.PROTOTYPES
        assert hasattr(abi.lib(), name)
    assert abi.lib().pcc_abi_version() == 1
    for word in ("k_eff = min(k, n_f)", "its own nearest neighbour", "row -1 and d2 = 2^64 - 1", "xx, xy, xz, yy, yz, zz",
                 "C = m * sum d_j d_j^T - (sum d_j)(sum d_j)^T", "smallest eigenvalue", "n . (viewpoint - p) < 0",
                 "(ex*nx + ey*ny) + ez*nz", "normal of the pair's A point"):      # the rules, in full
        assert word in text, word


def test_restatement_hand_worked():
    """Five points; biased by 32768 their low key bits are (0,0,0) -> 0, (0,1,0) -> 2, (1,0,0) -> 4, (1,1,0) -> 6,
    (0,0,2) -> 8, which is their Morton order: rows 0 .. 4.
    Row 0, k = 3: itself (0), then rows 1 and 2 at distance 1 (row 3 at 2 stays out).  d = (0,0,0), (0,1,0), (1,0,0):
    sum d = (1,1,0), sum d d^T = diag(1,1,0), so C = 3 diag(1,1,0) - (1,1,0)(1,1,0)^T: xx 2, xy -1, yy 2, rest 0.  The
    normal is (0,0,+-1), eigenvalue 0.
    Row 4 = (0,0,2), k = 3: itself, row 0 at 4, then rows 1 and 2 both at 5: the smaller row, 1.  d = (0,0,0), (0,0,-2),
    (0,1,-2): sum d = (0,1,-4), sum d d^T has yy 1, yz -2, zz 8; C: yy 3 - 1 = 2, yz -6 + 4 = -2, zz 24 - 16 = 8, rest 0.
    The normal is (+-1,0,0)."""
    pts = nn_ref.morton_sorted_unique([[1, 1, 0], [0, 0, 2], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert pts.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [0, 0, 2]]
    rows, d2 = normals_ref.knn(pts, 3)
    assert rows[0].tolist() == [0, 1, 2] and d2[0].tolist() == [0, 1, 1] and d2.dtype == np.uint64
    assert rows[4].tolist() == [4, 0, 1] and d2[4].tolist() == [0, 4, 5]
    c = normals_ref.scatter(pts, rows)
    assert c[0].tolist() == [2, -1, 0, 2, 0, 0] and c[4].tolist() == [0, 0, 0, 2, -2, 8] and c.dtype == np.int64
    n = normals_ref.normals_of(c)
    assert abs(abs(n[0, 2]) - 1) < 1e-6 and abs(abs(n[4, 0]) - 1) < 1e-6 and n.dtype == np.float32
    assert normals_ref.normals_of(c, pts, (0, 0, 9))[0, 2] > 0 and normals_ref.normals_of(c, pts, (0, 0, -9))[0, 2] < 0
    rows, d2 = normals_ref.knn(pts, 8)      # k_eff = 5
    assert rows[0].tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and d2[0].tolist() == [0, 1, 1, 2, 4] + [normals_ref.NO_DIST] * 3
    rows, _, c = normals_ref.knn_frames([pts[:2], pts], 3)      # rows over the call; 2 points: no normal, C = 0
    assert rows[:2].tolist() == [[0, 1, -1], [1, 0, -1]] and rows[2].tolist() == [2, 3, 4] and not c[:2].any()
    # D2: a at the origin with normal (0, 0, 1), its nearest b one up and one aside: only the part along the normal
    rep = normals_ref.d2([[0, 0, 0]], [[1, 0, 1]], [[0, 0, 1]], peak=3)
    assert rep["d2_mse_ab"] == 1.0 and rep["d2_mse_ba"] == 1.0 and abs(rep["d2_psnr"] - 10 * math.log10(27)) < 1e-12
    assert normals_ref.proj([[3, 4, 5]], [[1, 1, 1]], [[0.5, 0.25, -1]]).tolist() == [(1.0 + 0.75 - 4.0) ** 2]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_solver_passes_the_rayleigh_check(cases, name):
    case = cases[name]
    for k in KS:
        cov = case.expected(k)[2]
        assert normals_ref.rayleigh_check(cov[case.has_normal], normals_ref.normals_of(cov)[case.has_normal]) == 0
    # and the check refuses a wrong eigenvector: the middle one of a matrix with three separate eigenvalues
    c = np.array([[2, 0, 0, 5, 0, 9]])
    assert normals_ref.rayleigh_check(c, [[1, 0, 0]]) == 0 and normals_ref.rayleigh_check(c, [[0, 1, 0]]) == 1
    assert normals_ref.rayleigh_check(c, [[2, 0, 0]]) == 1 and normals_ref.rayleigh_check(c, [[np.nan, 0, 0]]) == 1


# (sum, max) of the nodes pcc_knn_replay_host reports per case at k = 3, 8, 16, 32, recorded from the library built at
# commit 4c134a5 (the last one with a walk of its own in knn.hip): the shared walk has to visit what that one visited
NODES_AT_4C134A5 = {
    "frame sizes": {3: (376786, 595), 8: (648341, 752), 16: (932665, 968), 32: (1345727, 1217)},
    "ties": {3: (33094, 228), 8: (56459, 298), 16: (78063, 332), 32: (109559, 387)},
    "range and pruning": {3: (114263, 361), 8: (190162, 459), 16: (281353, 545), 32: (430385, 654)},
    "flat": {3: (2275, 73), 8: (3131, 79), 16: (4078, 79), 32: (5176, 79)},
}


def _replay(keys, k):
    lib = pkg("_abi").lib()
    keys = np.ascontiguousarray(keys, np.uint64)
    n = keys.shape[0]
    w = max(k, 1)      # a refused k writes nothing
    rows, d2, cov = np.zeros((n, w), np.int32), np.zeros((n, w), np.uint64), np.zeros((n, 6), np.int64)
    normals, nodes = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    rc = lib.pcc_knn_replay_host(keys.ctypes.data, n, k, rows.ctypes.data, d2.ctypes.data, cov.ctypes.data, normals.ctypes.data,
                                 nodes.ctypes.data)
    return rc, rows, d2, cov, normals, nodes


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(CASES))
def test_traversal_replayed_on_the_host(cases, name, k):
    """the kernel's search and epilogue, compiled for the host, against the restatement; a query tries no more nodes
    than its frame's octree has (at most 16 per row) beside its k seeds, and the case as many as recorded"""
    case = cases[name]
    want_rows, want_d2, want_cov = case.expected(k)
    rc, rows, d2, cov, normals, nodes = _replay(case.keys, k)
    assert rc == 0
    assert np.array_equal(rows, want_rows) and np.array_equal(d2, want_d2) and np.array_equal(cov, want_cov)
    _check_normals(case, cov, normals)
    per_point = np.concatenate([np.full(f.shape[0], f.shape[0]) for f in case.frames])
    assert np.all(nodes <= k + 16 * per_point) and np.all(nodes >= np.minimum(k, per_point))
    assert (int(nodes.sum(dtype=np.uint64)), int(nodes.max())) == NODES_AT_4C134A5[name][k]


def test_replay_refusals():
    abi = pkg("_abi")
    lo, hi = [-32768] * 3, [32767] * 3
    rc, rows, d2, cov, normals, _ = _replay(nn_ref.morton_keys([lo, hi]), 3)      # two points: neighbours, no normal
    assert rc == 0 and rows.tolist() == [[0, 1, -1], [1, 0, -1]] and d2[0].tolist() == [0, 3 * 65535 ** 2, normals_ref.NO_DIST]
    assert not cov.any() and not normals.any()
    for k in (2, 33, 0, -1):
        rc, *_ = _replay(nn_ref.morton_keys([lo, hi]), k)
        assert rc == abi.PCC_E_ARG and b"k in 3 .. 32" in abi.lib().pcc_last_error()
    rc, *_ = _replay(nn_ref.morton_keys([hi, lo]), 3)
    assert rc == abi.PCC_E_ARG and b"not sorted" in abi.lib().pcc_last_error()
    rc, *_ = _replay(nn_ref.morton_keys([hi, hi]), 3)
    assert rc == abi.PCC_E_DUP and b"duplicate" in abi.lib().pcc_last_error()
    assert _replay(np.zeros(0, np.uint64), 3)[0] == 0


def test_normals_refusals_without_a_device():
    """the checks in front of the first use of the device: a codec object without a Runtime reaches them"""
    GeometryCodec = pkg().GeometryCodec
    geo = GeometryCodec.__new__(GeometryCodec)
    pts = np.array([[0, 0, 0], [1, 2, 3], [4, 5, 7]], np.int32)
    unit = np.tile(np.array([[0, 0, 1]], np.float32), (3, 1))
    for k in (2, 33, 16.0, True, None):
        with pytest.raises(ValueError, match="k must be an integer in 3 .. 32"):
            geo.normals([pts], k=k)
        with pytest.raises(ValueError, match="normal_k must be an integer in 3 .. 32"):
            geo.distortion([pts], [pts], normals_a="estimate", normal_k=k)
    for vp in ((1, 2), (1, 2, 3.5), 7, (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="viewpoint must be three integers"):
            geo.normals([pts], viewpoint=vp)
    with pytest.raises(TypeError, match="lattice points"):
        geo.normals([pts.astype(np.float32)])
    with pytest.raises(ValueError, match="output"):
        geo.normals([pts], output="torch")
    assert geo.normals([]) == []
    with pytest.raises(ValueError, match="'estimate'"):
        geo.distortion([pts], [pts], normals_a="guess")
    with pytest.raises(ValueError, match="2 normal arrays for 1 frames"):
        geo.distortion([pts], [pts], normals_a=[unit, unit])
    with pytest.raises(TypeError, match="frame 0: expected float32 normals, got float64"):
        geo.distortion([pts], [pts], normals_a=[unit.astype(np.float64)])
    with pytest.raises(ValueError, match=r"frame 0: expected normals of shape \[n, 3\]"):
        geo.distortion([pts], [pts], normals_a=[unit[:, :2]])
    with pytest.raises(ValueError, match="frame 1: 2 normals for 3 points"):
        geo.distortion([pts, pts], [pts, pts], normals_a=[unit, unit[:2]])
    bad = unit.copy()
    bad[1, 1] = np.inf
    with pytest.raises(ValueError, match="frame 0: non-finite normal"):
        geo.distortion([pts], [pts], normals_a=[bad])
    assert geo.distortion([], [], normals_a="estimate") == []


# ------------------------------------------------------------------ GPU: Runtime.knn_frames
def _dev(rt, keys):
    import torch
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(rt.device)


def _knn(rt, case, k, **kw):
    rows, d2, cov, normals = rt.knn_frames(_dev(rt, case.keys), len(case.frames), k, want_rows=True, want_dist=True,
                                           want_cov=True, **kw)
    rt.sync()
    return rows.cpu().numpy(), d2.cpu().numpy().view(np.uint64), cov.cpu().numpy(), normals.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(CASES))
def test_knn_frames_against_brute_force(rt, cases, name, k):
    case = cases[name]
    want_rows, want_d2, want_cov = case.expected(k)
    rows, d2, cov, normals = _knn(rt, case, k)
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(d2, want_d2)
    assert np.array_equal(cov, want_cov)
    _check_normals(case, cov, normals)


@pytest.mark.gpu
def test_knn_frames_outputs_are_optional(rt, cases):
    case = cases["ties"]
    keys = _dev(rt, case.keys)
    _, _, _, want = _knn(rt, case, 8)
    rows, d2, cov, normals = rt.knn_frames(keys, len(case.frames), 8)
    rt.sync()
    assert rows is None and d2 is None and cov is None and np.array_equal(normals.cpu().numpy(), want)
    rows, d2, cov, normals = rt.knn_frames(keys, len(case.frames), 8, want_rows=True, want_normals=False)
    rt.sync()
    assert normals is None and np.array_equal(rows.cpu().numpy(), case.expected(8)[0])
    assert rt.knn_frames(keys[:0], 1, 8)[3].shape == (0, 3)


@pytest.mark.gpu
def test_knn_frames_plane_line_and_viewpoint(rt, cases):
    """k = 3 is left out for the plane: a grid point, one neighbour to its left and one to its right are collinear, and
    then every vector across that line is a right answer; from k = 8 on a neighbourhood of the grid spans the plane"""
    case = cases["flat"]
    plane = slice(0, 36)
    assert np.all(case.points[plane, 2] == 5) and len(case.frames[0]) == 36
    for k in (8, 16, 32):
        _, _, cov, normals = _knn(rt, case, k)
        assert np.all(np.abs(normals[plane, 2]) >= 1 - 1e-6), k
        _check_normals(case, cov, normals)      # the line too: finite, unit, in the eigenspace
        up = _knn(rt, case, k, viewpoint=(0, 0, 1000))[3]
        down = _knn(rt, case, k, viewpoint=(0, 0, -1000))[3]
        assert np.all(up[plane, 2] > 0) and np.all(down[plane, 2] < 0)
        assert np.array_equal(np.abs(up), np.abs(normals)) and np.array_equal(up[plane], -down[plane])


@pytest.mark.gpu
def test_knn_frames_refusals_launch_nothing(rt):
    import torch
    abi = pkg("_abi")
    pts = nn_ref.morton_sorted_unique(np.random.default_rng(4).integers(-50, 50, (200, 3)))
    good = nn_ref.morton_keys(pts)
    n = good.shape[0]
    bad = {"not sorted": (good[::-1], 1, 8, abi.PCC_E_ARG), "duplicate": (np.repeat(good, 2)[:n], 1, 8, abi.PCC_E_DUP),
           "frame index": (nn_ref.morton_keys(pts, 2), 2, 8, abi.PCC_E_RANGE), "k=2": (good, 1, 2, abi.PCC_E_ARG),
           "k=33": (good, 1, 33, abi.PCC_E_ARG), "n_frames=0": (good, 0, 8, abi.PCC_E_ARG),
           "n_frames=65536": (good, 65536, 8, abi.PCC_E_ARG)}
    for word, (keys, n_frames, k, code) in bad.items():
        rows = torch.full((n, max(k, 1)), 7, dtype=torch.int32, device=rt.device)
        normals = torch.full((n, 3), 7, dtype=torch.float32, device=rt.device)
        d = _dev(rt, keys)
        rc = rt.lib.pcc_knn_frames(rt.ctx, C.c_void_p(d.data_ptr()), n, n_frames, k, C.c_void_p(rows.data_ptr()), None, None,
                                   C.c_void_p(normals.data_ptr()), None)
        assert rc == code and word.encode() in rt.lib.pcc_last_error(), (word, rc, rt.lib.pcc_last_error())
        rt.sync()
        assert bool((rows == 7).all()) and bool((normals == 7).all())
        with pytest.raises(abi.PccError, match=word):
            rt.knn_frames(d, n_frames, k)
    rc = rt.lib.pcc_knn_frames(rt.ctx, None, (1 << 27) + 1, 1, 8, None, None, None, None, None)
    assert rc == abi.PCC_E_ARG and b"2^27" in rt.lib.pcc_last_error()


# ------------------------------------------------------------------ GPU: GeometryCodec.normals
@pytest.fixture(scope="module")
def geo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg().GeometryCodec()
    yield g
    g.close()


@pytest.mark.gpu
def test_normals_follow_the_input_rows(geo, cases):
    import torch
    rng = np.random.default_rng(41)
    case = cases["range and pruning"]
    surface = case.frames[2]
    shuffled = surface[rng.permutation(surface.shape[0])]
    twice = np.concatenate([shuffled, shuffled[:100]]).astype(np.int32)      # duplicate rows share their point's normal
    frames = [twice, np.zeros((0, 3), np.int32), case.frames[1].astype(np.int32)]
    host = geo.normals(frames, k=8)
    assert [h.shape for h in host] == [(1600, 3), (0, 3), (301, 3)] and all(h.dtype == np.float32 for h in host)
    assert np.array_equal(host[0][:100], host[0][1500:])
    # row i is the normal of input row i: the scatter matrix of that point passes the check with it
    cov = normals_ref.scatter(surface, normals_ref.knn(surface, 8)[0])
    at = {tuple(p): i for i, p in enumerate(surface.tolist())}
    own = np.array([at[tuple(p)] for p in twice.tolist()])
    assert normals_ref.rayleigh_check(cov[own], host[0]) == 0
    order = rng.permutation(1600)      # another row order, the same normals row by row
    assert np.array_equal(geo.normals([twice[order]], k=8)[0], host[0][order])
    dev = geo.normals([torch.from_numpy(f).to(geo.rt.device) for f in frames], k=8, output="device")
    assert all(isinstance(d, torch.Tensor) and d.device == geo.rt.device and d.dtype == torch.float32 for d in dev)
    assert all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(dev, host))
    assert all(np.array_equal(a, h) for a, h in zip(geo.normals([f.astype(np.int16) for f in frames[1:]], k=8), host[1:]))
    up = geo.normals(frames, k=8, viewpoint=(0, 0, 30000))
    e = np.array([0, 0, 30000]) - twice
    assert np.all((e * up[0].astype(np.float64)).sum(1) >= -1e-9) and np.array_equal(np.abs(up[0]), np.abs(host[0]))
    empty = geo.normals([np.zeros((0, 3), np.int32)] * 2)
    assert [e.shape for e in empty] == [(0, 3), (0, 3)]


@pytest.mark.gpu
def test_normals_refusals(geo):
    pts = np.array([[0, 0, 0], [1, 2, 3], [4, 5, 7], [1, 2, 3]], np.int32)
    with pytest.raises(ValueError, match="frame 1: 2 distinct points in frames"):
        geo.normals([pts, pts[[0, 1, 3]]])
    with pytest.raises(ValueError, match="frame 0: 1 distinct points in frames"):
        geo.normals([pts[:1], pts])
    with pytest.raises(ValueError, match="k must be an integer in 3 .. 32"):
        geo.normals([pts], k=2)
    with pytest.raises(TypeError, match="lattice points"):
        geo.normals([pts.astype(np.float32)])
    with pytest.raises(pkg("_abi").PccError, match="outside"):
        geo.normals([pts + 40000])
    with pytest.raises(ValueError, match="frame 0: 2 distinct points in frames_a"):
        geo.distortion([pts[:2]], [pts], normals_a="estimate")
    assert geo.normals([pts])[0].shape == (4, 3)


# ------------------------------------------------------------------ GPU: D2
def _grid():
    g = 4 * np.arange(16)
    return np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2), np.zeros((256, 1), np.int64)], 1).astype(np.int32)


@pytest.mark.gpu
def test_d2_known_answers(geo):
    a = _grid()
    up = [np.tile(np.array([[0, 0, 1]], np.float32), (256, 1))]
    rep = geo.distortion([a], [a + np.array([1, 0, 0], np.int32)], normals_a=up, peak=63)[0]
    assert rep["mse_ab"] == 1.0 and rep["d2_mse_ab"] == 0.0 and rep["d2_mse_ba"] == 0.0 and rep["d2_psnr"] == float("inf")
    rep = geo.distortion([a], [a + np.array([0, 0, 3], np.int32)], normals_a=up, peak=63)[0]
    assert rep["mse_ab"] == 9.0 and rep["mse_ba"] == 9.0 and rep["d2_mse_ab"] == 9.0 and rep["d2_mse_ba"] == 9.0
    assert rep["d2_psnr"] == rep["d1_psnr"] == float(10.0 * np.log10(3.0 * 63.0 ** 2 / 9.0))
    for shift, want in (([1, 0, 0], 0.0), ([0, 0, 3], 9.0)):
        rep = geo.distortion([a], [a + np.array(shift, np.int32)], normals_a="estimate", normal_k=8)[0]
        assert abs(rep["d2_mse_ab"] - want) <= 1e-9 and abs(rep["d2_mse_ba"] - want) <= 1e-9 and rep["d2_psnr"] is None


@pytest.fixture(scope="module")
def lossy():
    """a surface cloud of 1 500 points, its lod-2 centres, random unit normals, and the restatement's answer"""
    rng = np.random.default_rng(51)
    a = surface_cloud(rng, 1500)[:, 1:]
    a = a[rng.permutation(a.shape[0])].astype(np.int32)
    b = nn_ref.morton_sorted_unique(((a >> 2) << 2) + 2).astype(np.int32)
    n = rng.normal(size=(a.shape[0], 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return a, b, n, normals_ref.d2(a, b, n, peak=255)


def _sum_bound(proj, extra=0):
    """summing non-negative float64 terms in any order stays within count 2^-52 of their exact sum; extra: further
    roundings between that sum and the figure compared (a report's mse is sum / count, and the test multiplies back)"""
    return (proj.shape[0] + extra) * 2.0 ** -52 * math.fsum(proj.tolist())


@pytest.mark.gpu
def test_nn_d2_frames_against_the_restatement(rt, lossy):
    import torch
    a, b, n, want = lossy
    order = np.argsort(nn_ref.morton_keys(a), kind="stable")
    akeys, bkeys = _dev(rt, nn_ref.morton_keys(a)[order]), _dev(rt, nn_ref.morton_keys(b))      # b is in Morton order
    normals = torch.from_numpy(n[order]).to(rt.device)
    _, row_ab, _ = rt.nn_frames(akeys, bkeys, 1, want_dist=False)
    _, row_ba, _ = rt.nn_frames(bkeys, akeys, 1, want_dist=False)
    proj, sums = rt.nn_d2_frames(akeys, row_ab, bkeys, normals, 1, want_proj=True)
    assert np.array_equal(proj.cpu().numpy(), want["proj_ab"][order])      # bit for bit
    assert abs(sums[0] - math.fsum(want["proj_ab"].tolist())) <= _sum_bound(want["proj_ab"])
    proj, sums = rt.nn_d2_frames(bkeys, row_ba, akeys, normals, 1, normal_row=row_ba, want_proj=True)
    assert np.array_equal(proj.cpu().numpy(), want["proj_ba"])
    assert abs(sums[0] - math.fsum(want["proj_ba"].tolist())) <= _sum_bound(want["proj_ba"])
    assert rt.nn_d2_frames(bkeys, row_ba, akeys, normals, 1, normal_row=row_ba)[0] is None
    # a row of -1 or outside the reference adds nothing, another frame's sum stays 0
    row_bad = row_ab.clone()
    row_bad[::2] = -1
    row_bad[1::4] = b.shape[0]
    proj, sums = rt.nn_d2_frames(akeys, row_bad, bkeys, normals, 2, want_proj=True)
    keep = np.ones(a.shape[0], bool)
    keep[::2] = False
    keep[1::4] = False
    kept = want["proj_ab"][order] * keep
    assert np.array_equal(proj.cpu().numpy(), kept) and abs(sums[0] - math.fsum(kept.tolist())) <= _sum_bound(kept) and sums[1] == 0.0


@pytest.mark.gpu
def test_per_frame_rounds_of_a_mixed_wave(rt):
    """the reduction that pcc_nn_frames, pcc_nn_attr_sse_frames and pcc_nn_d2_frames share, on the smallest shape in
    which its rounds per frame, its choice of a leader and a partial wave can go wrong together: 70 queries (one full
    wave and 6 lanes of a second), three frames interleaved lane by lane, frame 1 without a reference (all of its
    lanes are invalid, lane 1 among them) and one query of frame 0 whose row is taken away"""
    import torch
    rng = np.random.default_rng(61)
    q = rng.integers(-20, 20, (70, 3))
    frame = np.arange(70) % 3
    refs = [nn_ref.morton_sorted_unique(rng.integers(-20, 20, (25, 3))), np.zeros((0, 3), np.int64),
            nn_ref.morton_sorted_unique(rng.integers(-20, 20, (9, 3)))]
    d2s, rows, stats = nn_ref.nn_frames([q[frame == f] for f in range(3)], refs)
    want_d2, want_row = np.zeros(70, np.uint64), np.zeros(70, np.int64)
    for f in range(3):
        want_d2[frame == f], want_row[frame == f] = d2s[f], rows[f]
    assert stats[1] == [0, 0, 0] and np.all(want_row[frame == 1] == -1) and stats[0][0] == 24 and stats[2][0] == 23
    qkeys = _dev(rt, np.concatenate([nn_ref.morton_keys(q[i:i + 1], int(frame[i])) for i in range(70)]))
    rkeys = _dev(rt, np.concatenate([nn_ref.morton_keys(r, f) for f, r in enumerate(refs)]))
    sqdist, row, got_stats = rt.nn_frames(qkeys, rkeys, 3)
    assert np.array_equal(sqdist.cpu().numpy().view(np.uint64), want_d2) and np.array_equal(row.cpu().numpy(), want_row)
    assert got_stats == stats
    want_row[3] = -1      # lane 3, frame 0: the wave's first round loses a lane behind its leader
    row[3] = -1
    keep = want_row >= 0
    rpts = np.concatenate(refs)
    a, b = rng.integers(0, 256, (70, 3)).astype(np.uint8), rng.integers(0, 256, (rpts.shape[0], 3)).astype(np.uint8)
    a[0], b[:] = 255, 0      # the largest difference, whichever row the first query gets
    sq = (a.astype(np.int64) - b.astype(np.int64)[np.where(keep, want_row, 0)]) ** 2 * keep[:, None]
    got = rt.nn_attr_sse_frames(qkeys, row, torch.from_numpy(a).to(rt.device), torch.from_numpy(b).to(rt.device), 3)
    assert got == [[int(v) for v in sq[frame == f].sum(0)] for f in range(3)] and got[1] == [0, 0, 0]
    n = rng.normal(size=(70, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    want_proj = normals_ref.proj(q, rpts[np.where(keep, want_row, 0)], n) * keep
    proj, sums = rt.nn_d2_frames(qkeys, row, rkeys, torch.from_numpy(n).to(rt.device), 3, want_proj=True)
    assert np.array_equal(proj.cpu().numpy(), want_proj)      # bit for bit
    for f in range(3):
        mine = want_proj[frame == f]
        assert abs(sums[f] - math.fsum(mine.tolist())) <= _sum_bound(mine), f
    assert sums[1] == 0.0 and sums[0] > 0 and sums[2] > 0


@pytest.mark.gpu
def test_distortion_d2_against_the_restatement(geo, lossy):
    a, b, n, want = lossy
    today = geo.distortion([a], [b], peak=255)[0]
    assert set(today) == {"points_a", "points_b", "mse_ab", "mse_ba", "max_ab", "max_ba", "d1_psnr"}
    d1 = nn_ref.d1(a, b, 255)
    assert all(today[key] == d1[key] for key in d1)      # normals_a=None: the keys and values of before
    rep = geo.distortion([a], [b], peak=255, normals_a=[n])[0]
    assert {key: rep[key] for key in today} == today and set(rep) == set(today) | {"d2_mse_ab", "d2_mse_ba", "d2_psnr"}
    for name, count in (("ab", a.shape[0]), ("ba", b.shape[0])):
        assert abs(rep["d2_mse_" + name] * count - math.fsum(want["proj_" + name].tolist())) <= _sum_bound(want["proj_" + name], 2)
    assert rep["d2_psnr"] == float(10.0 * np.log10(3.0 * 255.0 ** 2 / max(rep["d2_mse_ab"], rep["d2_mse_ba"])))
    assert abs(rep["d2_psnr"] - want["d2_psnr"]) <= 1e-9
    assert rep["d2_mse_ab"] < rep["mse_ab"] and rep["d2_mse_ba"] < rep["mse_ba"]      # a projection is no longer than its vector
    with pytest.raises(ValueError, match="frame 0: 1 duplicate points in frames_a"):
        geo.distortion([np.concatenate([a, a[:1]])], [b], normals_a=[np.concatenate([n, n[:1]])])


@pytest.mark.gpu
def test_distortion_d2_frame_by_frame(geo, lossy):
    """a call of 3 frames equals three calls of 1.  Given normals with entries of a few bits make every proj a small
    multiple of 1/16, so the sums are exact in any order and equality is the right demand; estimated normals
    (duplicates on side A included) are held to the bound of the summation"""
    import torch
    a, b, _, _ = lossy
    rng = np.random.default_rng(52)
    fa = [a, a[:700] + np.array([40, 0, -7], np.int32), a[700:]]
    fb = [b, np.unique(((fa[1] >> 1) << 1) + 1, axis=0), np.unique(((fa[2] >> 3) << 3) + 4, axis=0)]
    dyadic = [rng.integers(-4, 5, (f.shape[0], 3)).astype(np.float32) / 4 for f in fa]
    whole = geo.distortion(fa, fb, peak=255, normals_a=dyadic)
    for f in range(3):
        assert geo.distortion(fa[f:f + 1], fb[f:f + 1], peak=255, normals_a=dyadic[f:f + 1])[0] == whole[f]
        assert whole[f]["d2_mse_ab"] > 0
    fa[1] = np.concatenate([fa[1], fa[1][:50]])      # duplicates on side A count, with their point's normal
    whole = geo.distortion(fa, fb, peak=255, normals_a="estimate", normal_k=8)
    dev = geo.distortion([torch.from_numpy(f).to(geo.rt.device) for f in fa], [torch.from_numpy(f).to(geo.rt.device) for f in fb],
                         peak=255, normals_a="estimate", normal_k=8)
    normals = geo.normals(fa, k=8)
    for f in range(3):
        one = geo.distortion(fa[f:f + 1], fb[f:f + 1], peak=255, normals_a="estimate", normal_k=8)[0]
        rb = nn_ref.morton_sorted_unique(fb[f])
        proj_ab = normals_ref.proj(fa[f], rb[nn_ref.nn(fa[f], rb)[1]], normals[f])
        for rep in (whole[f], one, dev[f]):
            assert all(rep[key] == one[key] for key in ("points_a", "points_b", "mse_ab", "mse_ba", "max_ab", "max_ba", "d1_psnr"))
            assert abs(rep["d2_mse_ab"] * fa[f].shape[0] - math.fsum(proj_ab.tolist())) <= _sum_bound(proj_ab, 2)
            # B -> A: both figures are within (count + 1) 2^-52 of the exact mean, so within twice that of one another
            assert abs(rep["d2_mse_ba"] - one["d2_mse_ba"]) <= 2 * (fb[f].shape[0] + 1) * 2.0 ** -52 * max(rep["d2_mse_ba"], one["d2_mse_ba"])
