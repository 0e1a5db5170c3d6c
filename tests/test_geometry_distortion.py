"""GeometryCodec.distortion and pcc_nn_frames: exact nearest neighbours on the lattice (include/pcc.h has the rule,
tests/nn_ref.py restates it by brute force).  Everything is held to equality: distances are integers.

CPU: the restatement worked by hand and against metrics._nn, the ABI, the traversal replayed on the host
(pcc_nn_replay_host is the kernel's search function compiled for the host), the refusals that need no device.
GPU: the kernel against the restatement on the smallest shapes at which it can go wrong.
"""
import ctypes as C
import os

import numpy as np
import pytest

import nn_ref
from conftest import ROOT, pkg, random_cloud, surface_cloud

CORNER_D2 = 12884508675      # 3 * 65535^2, above 2^32


# ------------------------------------------------------------------ shared cases (host arrays, computed once)
def _three_frames():
    """queries 1 / 257 / 3 000 rows (unsorted, with duplicates), references 1 / 64 / 2 999 distinct rows"""
    rng = np.random.default_rng(7)
    s = surface_cloud(rng, 257)[:, 1:]
    assert s.shape[0] == 257
    big = surface_cloud(rng, 1500)[:, 1:]
    base = np.concatenate([big, random_cloud(rng, 2800 - big.shape[0])[:, 1:]])
    q2 = np.concatenate([base, base[rng.integers(0, base.shape[0], 200)]])
    q2 = q2[rng.permutation(q2.shape[0])]
    assert q2.shape[0] == 3000 and np.unique(q2, axis=0).shape[0] < 3000
    queries = [np.array([[3, -4, 5]]), s[rng.permutation(257)], q2]
    refs = [np.array([[-7, 9, 2]]), random_cloud(rng, 64)[:, 1:], random_cloud(rng, 2999)[:, 1:]]
    return queries, [nn_ref.morton_sorted_unique(r) for r in refs]


def _seams():
    """one frame per seam s in 0, +-2, +-16, +-256: queries on both sides of it — (s-1, s-1, s-1) and (s, s, s) are
    adjacent in space and far apart in key order — and reference points on both sides too"""
    queries, refs = [], []
    for s in (0, 2, -2, 16, -16, 256, -256):
        queries.append(np.array([[s - 1] * 3, [s] * 3, [s - 1, s, s - 1]]))
        refs.append(nn_ref.morton_sorted_unique([[s - 2, s - 1, s - 1], [s + 1, s, s], [s - 1, s - 1, s - 3], [s, s + 2, s],
                                                 [s - 3, s - 3, s - 3], [s + 2, s + 2, s + 2]]))
    return queries, refs


def _ties():
    q = np.array([[10, -20, 30]])
    faces = q + np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    cube = q + np.array([[x, y, z] for x in (-3, 3) for y in (-3, 3) for z in (-3, 3)])
    origin = np.array([[0, 0, 0]])      # the same around the seam of all three axes
    cube0 = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)])
    return [q, q, origin], [nn_ref.morton_sorted_unique(r) for r in (faces, cube, cube0)]


def _worst():
    """a full 16^3 block in one corner of a 256-wide region, queries at the far corner and inside the block"""
    g = np.arange(16)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    far = 252 + np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    inside = np.random.default_rng(3).integers(0, 16, (64, 3))
    return [np.concatenate([far, inside])], [nn_ref.morton_sorted_unique(block)]


CASES = {"three frames": _three_frames, "seams": _seams, "ties": _ties, "worst case for pruning": _worst}


@pytest.fixture(scope="module")
def cases():
    """name -> (query keys uint64 [n_q] in a shuffled order, reference keys uint64 [n_r], n_frames, d2, row, stats)"""
    out = {}
    for name, make in CASES.items():
        queries, refs = make()
        d2s, rows, stats = nn_ref.nn_frames(queries, refs)
        qkeys = np.concatenate([nn_ref.morton_keys(q, f) for f, q in enumerate(queries)])
        rkeys = np.concatenate([nn_ref.morton_keys(r, f) for f, r in enumerate(refs)])
        assert np.all(np.diff(rkeys.astype(object)) > 0)
        order = np.random.default_rng(11).permutation(qkeys.shape[0])      # the frames of a call interleaved too
        out[name] = (qkeys[order], rkeys, len(queries), np.concatenate(d2s)[order], np.concatenate(rows)[order], stats)
    return out


# ------------------------------------------------------------------ CPU
def test_nn_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    for name in ("pcc_nn_frames", "pcc_nn_attr_sse_frames", "pcc_nn_replay_host"):
        assert name + "(" in text
        assert name in abi.PROTOTYPES
        assert hasattr(abi.lib(), name)
    assert abi.lib().pcc_abi_version() == 1
    for word in ("SMALLEST row", "d2 = 2^64 - 1 and row = -1", "12 884 508 675"):      # the rule, in full
        assert word in text, word


def test_restatement_hand_worked():
    """A = {(0,0,0), (1,0,0)}, B = {(0,0,0), (3,0,0)} (test_cpu's metric pair): A -> B distances (0, 1), sum 1;
    B -> A (0, 4), sum 4.  A tie: (1,0,0) between (0,0,0) and (2,0,0), both at distance 1; biased by 32768 their x are
    0x8000 and 0x8002, so (0,0,0) has the smaller key and is row 0: the Morton-first.  The opposite corners of the
    range differ by 65535 on every axis: d2 = 3 * 65535^2 = 12 884 508 675 > 2^32."""
    a, b = np.array([[0, 0, 0], [1, 0, 0]]), np.array([[0, 0, 0], [3, 0, 0]])
    d2, row = nn_ref.nn(a, nn_ref.morton_sorted_unique(b))
    assert d2.tolist() == [0, 1] and row.tolist() == [0, 0] and d2.dtype == np.uint64
    d2, row = nn_ref.nn(b, nn_ref.morton_sorted_unique(a))
    assert d2.tolist() == [0, 4] and row.tolist() == [0, 1]
    rep = nn_ref.d1(a, b, 7)
    assert (rep["mse_ab"], rep["mse_ba"], rep["max_ab"], rep["max_ba"]) == (0.5, 2.0, 1, 4)
    assert abs(rep["d1_psnr"] - 10 * np.log10(147 / 2)) < 1e-12
    ref = nn_ref.morton_sorted_unique([[2, 0, 0], [0, 0, 0]])
    assert ref.tolist() == [[0, 0, 0], [2, 0, 0]]
    d2, row = nn_ref.nn([[1, 0, 0]], ref)
    assert d2.tolist() == [1] and row.tolist() == [0]
    d2, row = nn_ref.nn([[-32768] * 3], [[32767] * 3])
    assert int(d2[0]) == CORNER_D2 == 3 * 65535 ** 2 and CORNER_D2 > 1 << 32
    d2s, rows, stats = nn_ref.nn_frames([[[1, 1, 1]], [[2, 2, 2]], [[0, 0, 0], [0, 0, 0]]], [[[1, 1, 2]], [], [[0, 3, 0]]])
    assert [d.tolist() for d in d2s] == [[1], [nn_ref.NO_DIST], [9, 9]] and [r.tolist() for r in rows] == [[0], [-1], [1, 1]]
    assert stats == [[1, 1, 1], [0, 0, 0], [2, 18, 9]]
    assert int(nn_ref.morton_keys([[-32768, -32768, -32767]], 3)[0]) == (3 << 48) | 1


def test_restatement_against_the_kd_tree():
    """metrics._nn (scipy's k-d tree, float64) on a random lattice cloud: the integer d2 recomputed from the tree's
    index equals the restatement's (the index itself may differ among equidistant points)"""
    rng = np.random.default_rng(5)
    a = rng.integers(-300, 300, (4000, 3))
    b = nn_ref.morton_sorted_unique(rng.integers(-300, 300, (3000, 3)))
    d2, row = nn_ref.nn(a, b)
    try:
        import scipy.spatial      # noqa: F401
        _, idx = pkg("metrics")._nn(a.astype(np.float64), b.astype(np.float64))
    except ImportError:      # a second brute force, chunked the other way round
        idx = np.concatenate([((a[i:i + 500, None, :] - b[None]) ** 2).sum(-1).argmin(1) for i in range(0, a.shape[0], 500)])
    assert np.array_equal(((a - b[idx]) ** 2).sum(1).astype(np.uint64), d2)
    assert np.array_equal(((a - b[row]) ** 2).sum(1).astype(np.uint64), d2)


# (sum, max) of the nodes pcc_nn_replay_host reports per case, recorded from the library built at commit 4c134a5 (the
# last one with a walk of its own in nn.hip): the shared walk has to visit what that one visited, node for node
NODES_AT_4C134A5 = {"three frames": (237153, 277), "seams": (432, 22), "ties": (61, 28), "worst case for pruning": (3008, 45)}


def _replay(qkeys, rkeys):
    lib = pkg("_abi").lib()
    qkeys, rkeys = np.ascontiguousarray(qkeys, np.uint64), np.ascontiguousarray(rkeys, np.uint64)
    d2, row, nodes = np.zeros(qkeys.shape[0], np.uint64), np.zeros(qkeys.shape[0], np.int32), np.zeros(qkeys.shape[0], np.uint32)
    rc = lib.pcc_nn_replay_host(qkeys.ctypes.data, qkeys.shape[0], rkeys.ctypes.data, rkeys.shape[0], d2.ctypes.data,
                                row.ctypes.data, nodes.ctypes.data)
    return rc, d2, row, nodes


@pytest.mark.parametrize("name", list(CASES))
def test_traversal_replayed_on_the_host(cases, name):
    """the kernel's search function, compiled for the host, against the restatement; a query tries no more nodes than
    its frame's octree has (at most 16 per reference row, and the two seeds), and the case as many as recorded"""
    qkeys, rkeys, n_frames, d2, row, _ = cases[name]
    rc, got_d2, got_row, nodes = _replay(qkeys, rkeys)
    assert rc == 0
    assert np.array_equal(got_d2, d2) and np.array_equal(got_row, row)
    per_frame = np.bincount((rkeys >> np.uint64(48)).astype(np.int64), minlength=n_frames)
    assert np.all(nodes <= 2 + 16 * per_frame[(qkeys >> np.uint64(48)).astype(np.int64)])
    assert (int(nodes.sum(dtype=np.uint64)), int(nodes.max())) == NODES_AT_4C134A5[name]


def test_replay_corners_and_refusals():
    lo, hi = [-32768] * 3, [32767] * 3
    rc, d2, row, _ = _replay(nn_ref.morton_keys([lo, hi, lo]), nn_ref.morton_keys([hi]))
    assert rc == 0 and d2.tolist() == [CORNER_D2, 0, CORNER_D2] and row.tolist() == [0, 0, 0]
    rc, d2, row, _ = _replay(nn_ref.morton_keys([lo], 1), nn_ref.morton_keys([hi], 0))      # another frame: no candidate
    assert rc == 0 and d2.tolist() == [nn_ref.NO_DIST] and row.tolist() == [-1]
    abi = pkg("_abi")
    rc, *_ = _replay(nn_ref.morton_keys([lo]), nn_ref.morton_keys([hi, lo]))
    assert rc == abi.PCC_E_ARG and b"not sorted" in abi.lib().pcc_last_error()
    rc, *_ = _replay(nn_ref.morton_keys([lo]), nn_ref.morton_keys([hi, hi]))
    assert rc == abi.PCC_E_DUP and b"duplicate" in abi.lib().pcc_last_error()


def test_distortion_refusals_without_a_device():
    """the checks in front of the first use of the device: a codec object without a Runtime reaches them"""
    GeometryCodec = pkg().GeometryCodec
    geo = GeometryCodec.__new__(GeometryCodec)
    pts = np.array([[0, 0, 0], [1, 2, 3]], np.int32)
    with pytest.raises(TypeError, match="lattice points"):
        geo.distortion([pts.astype(np.float32)], [pts])
    with pytest.raises(TypeError, match="lattice points"):
        geo.distortion([pts], [pts.astype(np.float32)])
    with pytest.raises(TypeError, match="float64"):
        geo.distortion([pts.astype(np.float64)], [pts])
    with pytest.raises(ValueError, match="1 frames against 2"):
        geo.distortion([pts], [pts, pts])
    with pytest.raises(ValueError, match="frame 1: 2 points against 0"):
        geo.distortion([pts, pts], [pts, pts[:0]])
    with pytest.raises(ValueError, match="one side only"):
        geo.distortion([pts], [pts], attributes_a=[np.zeros(2, np.uint8)])
    with pytest.raises(ValueError, match="frame 0: uint8 attributes of 1 channels against uint16"):
        geo.distortion([pts], [pts], attributes_a=[np.zeros(2, np.uint8)], attributes_b=[np.zeros(2, np.uint16)])
    with pytest.raises(ValueError, match="peak"):
        geo.distortion([pts], [pts], peak=0)
    assert geo.distortion([], []) == []


# ------------------------------------------------------------------ GPU: Runtime.nn_frames
def _dev(rt, keys):
    import torch
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(rt.device)


def _run(rt, qkeys, rkeys, n_frames, **kw):
    sqdist, row, stats = rt.nn_frames(_dev(rt, qkeys), _dev(rt, rkeys), n_frames, **kw)
    return (None if sqdist is None else sqdist.cpu().numpy().view(np.uint64), None if row is None else row.cpu().numpy(), stats)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shuffled", "sorted"])
@pytest.mark.parametrize("name", list(CASES))
def test_nn_frames_against_brute_force(rt, cases, name, order):
    qkeys, rkeys, n_frames, d2, row, stats = cases[name]
    if order == "sorted":
        by_key = np.argsort(qkeys, kind="stable")
        qkeys, d2, row = qkeys[by_key], d2[by_key], row[by_key]
    got_d2, got_row, got_stats = _run(rt, qkeys, rkeys, n_frames)
    assert np.array_equal(got_d2, d2)
    assert np.array_equal(got_row, row)
    assert got_stats == stats
    # the outputs are optional, and the statistics do not depend on which are asked for
    none_d2, only_row, stats2 = _run(rt, qkeys, rkeys, n_frames, want_dist=False)
    assert none_d2 is None and np.array_equal(only_row, row) and stats2 == stats
    assert _run(rt, qkeys, rkeys, n_frames, want_dist=False, want_row=False) == (None, None, stats)


@pytest.mark.gpu
def test_nn_frames_keeps_to_the_frame(rt):
    """frame 0's only reference point is far away, frame 1 holds a reference point equal to frame 0's query"""
    q = np.concatenate([nn_ref.morton_keys([[5, 5, 5]], 0), nn_ref.morton_keys([[5, 5, 5]], 1)])
    r = np.concatenate([nn_ref.morton_keys([[30000, -30000, 100]], 0), nn_ref.morton_keys([[5, 5, 5], [6, 5, 5]], 1)])
    far = 29995 ** 2 + 30005 ** 2 + 95 ** 2
    d2, row, stats = _run(rt, q, r, 2)
    assert d2.tolist() == [far, 0] and row.tolist() == [0, 1] and stats == [[1, far, far], [1, 0, 0]]
    # the last query of frame 0 in key order: its upper neighbour in key order is frame 1's first point
    q = np.concatenate([nn_ref.morton_keys([[32767, 32767, 32767]], 0), nn_ref.morton_keys([[-32768, -32768, -32768]], 1)])
    r = np.concatenate([nn_ref.morton_keys([[-32768, -32768, -32768]], 0), nn_ref.morton_keys([[-32768, -32768, -32768]], 1)])
    d2, row, stats = _run(rt, q, r, 2)
    assert d2.tolist() == [CORNER_D2, 0] and row.tolist() == [0, 1]


@pytest.mark.gpu
def test_nn_frames_range_corners(rt):
    lo, hi = [-32768] * 3, [32767] * 3
    q = np.concatenate([nn_ref.morton_keys([lo, lo], 0), nn_ref.morton_keys([hi], 1)])
    r = np.concatenate([nn_ref.morton_keys([hi], 0), nn_ref.morton_keys([lo], 1)])
    d2, row, stats = _run(rt, q, r, 2)
    assert d2.tolist() == [CORNER_D2] * 3 and row.tolist() == [0, 0, 1]
    assert stats == [[2, 2 * CORNER_D2, CORNER_D2], [1, CORNER_D2, CORNER_D2]]


@pytest.mark.gpu
def test_nn_frames_ties_take_the_smallest_row(rt, cases):
    qkeys, rkeys, n_frames, d2, row, _ = cases["ties"]
    _, got_row, _ = _run(rt, qkeys, rkeys, n_frames)
    firsts = np.searchsorted(rkeys, np.arange(n_frames, dtype=np.uint64) << np.uint64(48))
    assert sorted(got_row.tolist()) == sorted(firsts.tolist())      # every reference point ties: the frame's first row


@pytest.mark.gpu
def test_nn_frames_empty_sides(rt):
    pts = nn_ref.morton_sorted_unique(np.random.default_rng(2).integers(-50, 50, (300, 3)))
    none = np.zeros(0, np.uint64)
    d2, row, stats = _run(rt, none, nn_ref.morton_keys(pts), 2)
    assert d2.shape == (0,) and row.shape == (0,) and stats == [[0, 0, 0], [0, 0, 0]]
    d2, row, stats = _run(rt, nn_ref.morton_keys(pts[:70]), none, 2)
    assert d2.tolist() == [nn_ref.NO_DIST] * 70 and row.tolist() == [-1] * 70 and stats == [[0, 0, 0], [0, 0, 0]]
    assert _run(rt, none, none, 1)[2] == [[0, 0, 0]]
    # a frame empty on both sides between two full frames, and a frame with queries and no reference behind them
    queries = [pts[:100] + 1, pts[:0], pts[100:] + 2, pts[:5]]
    refs = [pts[::2], pts[:0], pts[1::2], pts[:0]]
    want_d2, want_row, want_stats = nn_ref.nn_frames(queries, refs)
    d2, row, stats = _run(rt, np.concatenate([nn_ref.morton_keys(q, f) for f, q in enumerate(queries)]),
                          np.concatenate([nn_ref.morton_keys(r, f) for f, r in enumerate(refs)]), 4)
    assert np.array_equal(d2, np.concatenate(want_d2)) and np.array_equal(row, np.concatenate(want_row))
    assert stats == want_stats and stats[1] == [0, 0, 0] and stats[3] == [0, 0, 0] and d2[-5:].tolist() == [nn_ref.NO_DIST] * 5


@pytest.mark.gpu
def test_nn_frames_refusals_launch_nothing(rt):
    import torch
    abi = pkg("_abi")
    pts = nn_ref.morton_sorted_unique(np.random.default_rng(4).integers(-50, 50, (200, 3)))
    good = nn_ref.morton_keys(pts)
    q = _dev(rt, good[:50])
    bad = {"not sorted": (good[::-1], 1, abi.PCC_E_ARG), "duplicate": (np.repeat(good, 2), 1, abi.PCC_E_DUP),
           "reference key's frame index": (nn_ref.morton_keys(pts, 2), 2, abi.PCC_E_RANGE)}
    for word, (rkeys, n_frames, code) in bad.items():
        sqdist = torch.full((50,), 7, dtype=torch.int64, device=rt.device)
        row = torch.full((50,), 7, dtype=torch.int32, device=rt.device)
        stats = torch.zeros((n_frames, 3), dtype=torch.int64, device=rt.device)
        r = _dev(rt, rkeys)
        rc = rt.lib.pcc_nn_frames(rt.ctx, C.c_void_p(q.data_ptr()), 50, C.c_void_p(r.data_ptr()), r.shape[0], n_frames,
                                  C.c_void_p(sqdist.data_ptr()), C.c_void_p(row.data_ptr()), C.c_void_p(stats.data_ptr()))
        assert rc == code and word.encode() in rt.lib.pcc_last_error(), (word, rc, rt.lib.pcc_last_error())
        rt.sync()
        assert sqdist.cpu().tolist() == [7] * 50 and row.cpu().tolist() == [7] * 50 and not stats.cpu().any()
        with pytest.raises(abi.PccError, match=word):
            rt.nn_frames(q, r, n_frames)
    with pytest.raises(abi.PccError, match="query key's frame index"):
        rt.nn_frames(_dev(rt, nn_ref.morton_keys(pts, 1)), _dev(rt, good), 1)
    with pytest.raises(abi.PccError, match="n_frames=0"):
        rt.nn_frames(q, _dev(rt, good), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,channels", [(np.uint8, 3), (np.uint16, 1), (np.uint16, 4)])
def test_nn_attr_sse_frames(rt, dtype, channels):
    import torch
    rng = np.random.default_rng(9)
    queries = [rng.integers(-30, 30, (700, 3)), rng.integers(-30, 30, (1, 3)), rng.integers(-30, 30, (333, 3))]
    refs = [nn_ref.morton_sorted_unique(rng.integers(-30, 30, (n, 3))) for n in (500, 3, 65)]
    top = np.iinfo(dtype).max
    a = rng.integers(0, top + 1, (sum(q.shape[0] for q in queries), channels)).astype(dtype)
    b = rng.integers(0, top + 1, (sum(r.shape[0] for r in refs), channels)).astype(dtype)
    a[0], b[:] = top, 0      # the largest difference on the first query, whichever row it gets
    qkeys = _dev(rt, np.concatenate([nn_ref.morton_keys(q, f) for f, q in enumerate(queries)]))
    rkeys = _dev(rt, np.concatenate([nn_ref.morton_keys(r, f) for f, r in enumerate(refs)]))
    _, row, _ = rt.nn_frames(qkeys, rkeys, 3, want_dist=False)
    _, rows, _ = nn_ref.nn_frames(queries, refs)
    assert np.array_equal(row.cpu().numpy(), np.concatenate(rows))
    tdtype = torch.uint8 if dtype == np.uint8 else torch.uint16
    dev = lambda v: torch.from_numpy(v.view(np.uint8)).to(rt.device).view(tdtype).reshape(v.shape)      # noqa: E731
    got = rt.nn_attr_sse_frames(qkeys, row, dev(a), dev(b), 3)
    diff = (a.astype(np.int64) - b.astype(np.int64)[np.concatenate(rows)]) ** 2
    ends = np.cumsum([0] + [q.shape[0] for q in queries])
    assert got == [[int(v) for v in diff[s:e].sum(0)] for s, e in zip(ends[:-1], ends[1:])]


# ------------------------------------------------------------------ GPU: GeometryCodec.distortion
@pytest.fixture(scope="module")
def geo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _cloud(seed, n, extent=200, lo=-100):
    return random_cloud(np.random.default_rng(seed), n, extent=extent, lo=lo)[:, 1:].copy()


@pytest.mark.gpu
def test_distortion_of_a_lossless_round_trip_is_zero(geo):
    import torch
    frames = [_cloud(1, 1500), np.zeros((0, 3), np.int32), _cloud(2, 700).astype(np.int16)]
    frames[0] = np.concatenate([frames[0], frames[0][:40]])      # duplicates on the query side count, and cost nothing
    blobs = geo.compress([f.astype(np.int32) for f in frames])
    for a, b in ((frames, geo.decompress(blobs)),
                 ([torch.from_numpy(f.astype(np.int32)).to(geo.rt.device) for f in frames], geo.decompress(blobs, output="device"))):
        rep = geo.distortion(a, b, peak=255)
        assert [r["points_a"] for r in rep] == [1540, 0, 700] and [r["points_b"] for r in rep] == [1500, 0, 700]
        for r in rep:
            assert (r["mse_ab"], r["mse_ba"], r["max_ab"], r["max_ba"]) == (0.0, 0.0, 0, 0) and r["d1_psnr"] == float("inf")
            assert isinstance(r["max_ab"], int) and "attr_mse_ab" not in r
    assert geo.distortion(frames, geo.decompress(blobs))[0]["d1_psnr"] is None


@pytest.mark.gpu
def test_distortion_of_lod_centres(geo):
    """cells of lod k compared as their centres (c << k) + 2^(k-1): a point of the cell is off by at most 2^(k-1) <=
    2^k - 1 per axis, so max_ab <= 3 (2^k - 1)^2 whatever the data"""
    pts = [_cloud(3, 2000), _cloud(4, 600, extent=60, lo=-10)]
    blobs = geo.compress(pts)
    metrics = pkg("metrics")
    for k in (1, 2, 3):
        cells = geo.decompress(blobs, lod=k)
        centres = [(c << k) + ((1 << k) >> 1) for c in cells]
        rep = geo.distortion(pts, centres, peak=255)
        for f in range(2):
            want = nn_ref.d1(pts[f], centres[f], 255)
            for key in ("mse_ab", "mse_ba", "max_ab", "max_ba", "d1_psnr"):
                assert rep[f][key] == want[key], (k, f, key)
            assert 0 < rep[f]["max_ab"] <= 3 * ((1 << k) - 1) ** 2
            try:
                import scipy.spatial      # noqa: F401
                psnr = metrics.d1_psnr(pts[f], centres[f], 255)[0]
            except ImportError:
                psnr = want["d1_psnr"]
            assert abs(rep[f]["d1_psnr"] - psnr) <= 1e-12 * abs(psnr)


@pytest.mark.gpu
def test_distortion_with_attributes(geo):
    rng = np.random.default_rng(6)
    frames = [_cloud(5, 1200), _cloud(6, 333, extent=40, lo=-20)]
    attrs = [rng.integers(0, 256, (1200, 3)).astype(np.uint8), rng.integers(0, 65536, 333).astype(np.uint16)]
    blobs, exact = geo.compress(frames, attributes=attrs)
    _, lossy = geo.compress(frames, attributes=attrs, max_error=2)
    f0, a0 = geo.decompress(blobs, exact)
    f1, a1 = geo.decompress(blobs, lossy)
    rep = geo.distortion(f0, f1, attributes_a=a0, attributes_b=a1)
    for f in range(2):
        assert rep[f]["mse_ab"] == 0.0 and rep[f]["d1_psnr"] is None
        assert rep[f]["attr_mse_ab"] == nn_ref.attr_mse(f0[f], a0[f], f1[f], a1[f])
        assert rep[f]["attr_mse_ba"] == nn_ref.attr_mse(f1[f], a1[f], f0[f], a0[f])
        assert len(rep[f]["attr_mse_ab"]) == a0[f].shape[1] and 0 < max(rep[f]["attr_mse_ab"]) and max(rep[f]["attr_mse_ab"]) <= 4
        assert max(rep[f]["attr_mse_ba"]) <= 4
    # other geometry on the two sides, in the caller's row order: the values follow the sort and the nearest row
    sub = [f[::3] for f in frames]
    sub_attrs = [a[::3] for a in attrs]
    rep = geo.distortion(frames, sub, attributes_a=attrs, attributes_b=sub_attrs, peak=255)
    for f in range(2):
        assert rep[f]["attr_mse_ab"] == nn_ref.attr_mse(frames[f], attrs[f], sub[f], sub_attrs[f])
        assert rep[f]["attr_mse_ba"] == [0.0] * attrs[f].reshape(frames[f].shape[0], -1).shape[1]
        assert rep[f]["mse_ab"] == nn_ref.d1(frames[f], sub[f])["mse_ab"] and rep[f]["mse_ba"] == 0.0
    # duplicates on a side
    twice = [np.concatenate([frames[0], frames[0][:1]]), frames[1]]
    with pytest.raises(ValueError, match="frame 0: 1 duplicate points in frames_b"):
        geo.distortion(frames, twice, attributes_a=attrs, attributes_b=[np.concatenate([attrs[0], attrs[0][:1]]), attrs[1]])
    twice = [frames[0], np.concatenate([frames[1], frames[1][:2]])]
    with pytest.raises(ValueError, match="frame 1: 2 duplicate points in frames_a"):
        geo.distortion(twice, frames, attributes_a=[attrs[0], np.concatenate([attrs[1], attrs[1][:2]])], attributes_b=attrs)


@pytest.mark.gpu
def test_distortion_refusals(geo):
    pts = _cloud(8, 50)
    with pytest.raises(ValueError, match="frame 1: 0 points against 50"):
        geo.distortion([pts, pts[:0]], [pts, pts])
    with pytest.raises(TypeError, match="lattice points"):
        geo.distortion([pts.astype(np.float32)], [pts])
    with pytest.raises(pkg("_abi").PccError, match="outside"):
        geo.distortion([pts + 40000], [pts])
    import torch
    with pytest.raises(ValueError, match="host"):
        geo.distortion([torch.from_numpy(pts).to(geo.rt.device)], [pts])
    rep = geo.distortion([pts[:0]], [pts[:0]], peak=7)
    assert rep == [{"points_a": 0, "points_b": 0, "mse_ab": 0.0, "mse_ba": 0.0, "max_ab": 0, "max_ba": 0, "d1_psnr": float("inf")}]
