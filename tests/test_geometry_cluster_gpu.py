"""GeometryCodec.cluster and the clustering kernels on the device (csrc/cluster.h behind csrc/knn.hip, csrc/cluster.hip),
held integer for integer to tests/cluster_ref.py and to the host replay on the cases of tests/test_geometry_cluster.py:
the hand-worked frames, a mixed call of six frames, the parameter subset, every thread uniting into one root, long
parent chains, many small components on both routes of the sort, device tensors in and out, and the pipeline
filter -> cluster -> compress on the device.  Every shape but one is at most 20 000 points."""
import numpy as np
import pytest

import cluster_ref
import nn_ref
from conftest import pkg
from test_geometry_cluster import HAND, PARAMS, Call, _cloud, assert_same, hand, replay, sizes_call, snake_keys


def _dev(rt, keys):
    import torch
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(rt.device)


@pytest.fixture(scope="module")
def geo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg().GeometryCodec()
    yield g
    g.close()


def device(rt, keys, n_frames, m, radius2, min_points):
    """pcc_cluster_frames -> the replay's layout (without roots, which the device does not return)"""
    labels, sizes, counts = rt.cluster_frames(_dev(rt, keys), n_frames, m, radius2, min_points)
    counts = rt._u64_rows(counts)
    return {"labels": labels.cpu().numpy(), "sizes": sizes.cpu().numpy().view(np.uint32), "counts": counts}


def assert_device(got, want):
    assert np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(got["sizes"], want["sizes"])
    assert got["counts"] == want["counts"]


# ------------------------------------------------------------------ worked by hand
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_hand_worked_frames_on_the_device(geo, name):
    p, radius2, m, min_points, labels, sizes, (n_core, n_noise) = hand(name)
    (got,), (rep,) = geo.cluster([p.astype(np.int32)], radius2=radius2, min_neighbours=m, min_points=min_points, return_report=True)
    assert got.dtype == np.int32 and np.array_equal(got, labels)
    assert rep == {"points": p.shape[0], "core": n_core, "clusters": len(sizes), "noise": n_noise, "sizes": sizes}
    assert all(type(v) is int for v in list(rep.values())[:4] + rep["sizes"])


@pytest.mark.gpu
def test_edge_frames(geo):
    one = np.array([[3, -4, 5]], np.int16)
    none = np.zeros((0, 3), np.int16)
    labels, rep = geo.cluster([none, one], radius2=3, return_report=True)
    assert labels[0].shape == (0,) and labels[0].dtype == np.int32 and labels[1].tolist() == [0]
    assert rep == [{"points": 0, "core": 0, "clusters": 0, "noise": 0, "sizes": []},
                   {"points": 1, "core": 1, "clusters": 1, "noise": 0, "sizes": [1]}]
    labels, rep = geo.cluster([one, none], radius2=3, min_neighbours=1, return_report=True)
    assert labels[0].tolist() == [-1] and labels[1].shape == (0,)
    assert rep[0] == {"points": 1, "core": 0, "clusters": 0, "noise": 1, "sizes": []}
    assert [a.shape for a in geo.cluster([none, none], radius2=3)] == [(0,), (0,)]


# ------------------------------------------------------------------ a mixed call
def _mixed_frames():
    """0, 1, 2, 257, 9 000 and 9 000 rows; the fourth with every fifth row given twice, all shuffled"""
    rng = np.random.default_rng(51)
    d = _cloud(53, 257)
    d = np.concatenate([d, d[::5]])
    frames = [np.zeros((0, 3), np.int64), _cloud(51, 1), _cloud(52, 2), d, _cloud(54, 9000), _cloud(55, 9000)]
    return [f[rng.permutation(f.shape[0])] for f in frames]


@pytest.fixture(scope="module")
def mixed():
    frames = _mixed_frames()
    return frames, [cluster_ref.cluster_rows(f, 3, 2, 3) for f in frames]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "int32", "float32"])
@pytest.mark.parametrize("place", ["host", "device"])
def test_cluster_follows_the_input_rows(geo, mixed, place, dtype):
    import torch
    frames, want = mixed
    kw = dict(radius2=3, min_neighbours=2, min_points=3, return_report=True)
    if dtype == "float32":      # x = origin + q * voxel, exact in float32: the lattice is the same
        given = [(f * 0.25 + np.array([1.0, -2.0, 0.5])).astype(np.float32) for f in frames]
        kw.update(voxel=0.25, origin=(1.0, -2.0, 0.5))
    else:
        given = [f.astype(dtype) for f in frames]
    inputs = [torch.from_numpy(g).to(geo.rt.device) for g in given] if place == "device" else given
    labels, report = geo.cluster(inputs, **kw)
    for f, (w_rows, w) in enumerate(want):
        assert np.array_equal(labels[f], w_rows), f
        n, core, k, noise = w["counts"]
        assert report[f] == {"points": n, "core": core, "clusters": k, "noise": noise, "sizes": w["sizes"]}, f
    assert report[4]["clusters"] > 1 and report[4]["noise"] > 0 and report[4]["core"] < report[4]["points"]      # all of the rule is in play


@pytest.mark.gpu
def test_dropped_rows_are_noise(geo):
    """invalid="drop": a NaN row gets -1 and takes no part; the other rows' labels are those of the frame without it"""
    rows = (_cloud(61, 400) * 0.5).astype(np.float32)
    bad = rows.copy()
    bad[[0, 17, 399]] = [np.nan, 1.0, np.inf]
    kw = dict(radius2=3, min_neighbours=1, min_points=2, voxel=0.5)
    (got,) = geo.cluster([bad], invalid="drop", **kw)
    keep = np.ones(400, bool)
    keep[[0, 17, 399]] = False
    (want,) = geo.cluster([rows[keep]], **kw)
    assert np.array_equal(got[keep], want) and (got[~keep] == -1).all()
    assert np.array_equal(want, cluster_ref.cluster_rows(np.rint(rows[keep] / 0.5).astype(np.int64), 3, 1, 2)[0])
    with pytest.raises(pkg("_abi").PccError, match="non-finite"):
        geo.cluster([bad], **kw)
    assert geo.cluster([bad[[0, 17]]], invalid="drop", **kw)[0].tolist() == [-1, -1]      # nothing is left to cluster


# ------------------------------------------------------------------ the kernels against the replay
@pytest.mark.gpu
@pytest.mark.parametrize("radius2, m, min_points", PARAMS)
def test_device_against_the_replay(rt, radius2, m, min_points):
    c = sizes_call()
    want = replay(c.keys, len(c.frames), m, radius2, min_points)
    got = device(rt, c.keys, len(c.frames), m, radius2, min_points)
    assert_device(got, want)
    # the roots, which only the replay returns: a cluster's root is the first core row that carries its label
    core = want["core"] != 0
    for lo, hi in zip(c.first[:-1], c.first[1:]):
        labels = got["labels"][lo:hi]
        for label in np.unique(labels[labels >= 0]).tolist()[:20]:
            rows = lo + np.flatnonzero((labels == label) & core[lo:hi])
            assert (want["root"][rows] == rows[0]).all()


@pytest.mark.gpu
def test_contention_on_one_root(rt):
    """a dense 16^3 cube at radius2 = 3: every thread unites into the same root.  Run twice: the same, bit for bit"""
    g = np.arange(16)
    cube = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) - 8
    keys = np.sort(nn_ref.morton_keys(cube))
    first = device(rt, keys, 1, 0, 3, 1)
    assert first["counts"] == [[4096, 4096, 1, 0]] and first["sizes"][0] == 4096 and not first["sizes"][1:].any()
    assert not first["labels"].any()
    again = device(rt, keys, 1, 0, 3, 1)
    assert_device(again, first)
    assert_device(first, replay(keys, 1, 0, 3, 1))


@pytest.mark.gpu
def test_long_parent_chains(rt):
    keys = snake_keys()
    want = replay(keys, 1, 0, 1, 1)
    got = device(rt, keys, 1, 0, 1, 1)
    assert got["counts"] == [[20000, 20000, 1, 0]]
    assert_device(got, want)


def _lattice(n):
    """n points on a lattice of spacing 3 about the origin: at radius2 = 4 nobody has a neighbour"""
    e = int(np.ceil(n ** (1 / 3)))
    g = (np.arange(e) - e // 2) * 3
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9000, 70000])      # the sort's one-workgroup route and its multi-pass route (above 65 536)
def test_many_small_components(rt, n):
    """n clusters of one: every sort key is equal, so the numbering is the sort's stability — labels in row order"""
    keys = np.sort(nn_ref.morton_keys(_lattice(n)))
    got = device(rt, keys, 1, 0, 4, 1)
    assert got["counts"] == [[n, n, n, 0]]
    assert np.array_equal(got["labels"], np.arange(n, dtype=np.int32)) and (got["sizes"] == 1).all()
    got = device(rt, keys, 1, 0, 4, 2)
    assert got["counts"] == [[n, n, 0, n]] and (got["labels"] == -1).all() and not got["sizes"].any()


@pytest.mark.gpu
def test_frames_do_not_mix_on_the_device(rt):
    a, b = _cloud(41, 300), _cloud(42, 280)
    c = Call([a, b, a])
    for radius2, m, min_points in ((3, 0, 1), (12, 4, 2)):
        assert_device(device(rt, c.keys, 3, m, radius2, min_points), c.want(radius2, m, min_points))


# ------------------------------------------------------------------ device tensors, and the pipeline
@pytest.mark.gpu
def test_output_on_the_device(geo):
    import torch
    frames = [_cloud(71, 500).astype(np.int32), np.zeros((0, 3), np.int32), _cloud(72, 300).astype(np.int32)]
    kw = dict(radius2=3, min_neighbours=1, min_points=2, return_report=True)
    want, want_rep = geo.cluster(frames, **kw)
    got, rep = geo.cluster([torch.from_numpy(f).to(geo.rt.device) for f in frames], output="device", **kw)
    assert rep == want_rep
    for g, w in zip(got, want):
        assert isinstance(g, torch.Tensor) and g.device == geo.rt.device and g.dtype == torch.int32
        assert np.array_equal(g.cpu().numpy(), w)
    got = geo.cluster(frames, output="device", radius2=3, min_neighbours=1, min_points=2)      # host frames, device labels
    assert all(g.device == geo.rt.device and np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


@pytest.mark.gpu
def test_pipeline_on_the_device(geo):
    """filter -> cluster -> boolean index -> compress with no host array in between: the blobs of the same steps
    through numpy"""
    import torch
    def plate(e):      # e x e x 2 voxels, dense
        g = np.arange(e) - e // 2
        return np.stack(np.meshgrid(g, g, np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    g = np.arange(3)
    blob = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + [200, 200, 200]      # dense: filter keeps it
    far = np.array([[-300, 250, 90], [310, -310, 10]])      # flying pixels: filter's
    frames = [np.concatenate([plate(40), blob, far]).astype(np.int32), plate(30).astype(np.int32)]
    f_kw = dict(method="radius", min_neighbours=2, radius2=9)
    c_kw = dict(radius2=3, min_points=100)
    kept = geo.filter(frames, **f_kw)
    labels = geo.cluster(kept, **c_kw)
    want = geo.compress([k[l >= 0] for k, l in zip(kept, labels)])
    assert kept[0].shape[0] == 3200 + 27 and (labels[0] < 0).sum() == 27      # the blob went here, not in filter
    assert all((l[:900] == 0).all() for l in labels)
    dev = [torch.from_numpy(f).to(geo.rt.device) for f in frames]
    kept_d = geo.filter(dev, output="device", **f_kw)
    labels_d = geo.cluster(kept_d, output="device", **c_kw)
    got = geo.compress([k[l >= 0] for k, l in zip(kept_d, labels_d)])
    assert [bytes(b) for b in got] == [bytes(b) for b in want]


# ------------------------------------------------------------------ the largest radius, and the refusals
@pytest.mark.gpu
def test_largest_radius_and_refusals(geo, rt):
    abi = pkg("_abi")
    pts = nn_ref.morton_sorted_unique(_cloud(91, 2000) * 20)      # spread out: radius 64 is 3.2 steps of this lattice
    keys = nn_ref.morton_keys(pts)
    assert_device(device(rt, keys, 1, 1, 4096, 2), replay(keys, 1, 1, 4096, 2))
    (labels,) = geo.cluster([pts.astype(np.int32)], radius2=4096, min_neighbours=1, min_points=2)
    want = cluster_ref.cluster(pts, 4096, 1, 2)
    assert np.array_equal(labels, want["labels"]) and want["counts"][2] > 1 and want["counts"][3] > 0
    with pytest.raises(ValueError, match="radius2 must be an integer in 0 .. 4096"):
        geo.cluster([pts.astype(np.int32)], radius2=4097)
    d_keys = _dev(rt, keys)
    for kw, word in ((dict(radius2=4097), "radius2 in 0 .. 4096"), (dict(m=32), "min_neighbours in 0 .. 31"),
                     (dict(m=-1), "min_neighbours in 0 .. 31"), (dict(min_points=0), "min_points in 1 .. 2\\^27"),
                     (dict(min_points=(1 << 27) + 1), "min_points in 1 .. 2\\^27")):
        a = dict(m=0, radius2=3, min_points=1)
        a.update(kw)
        with pytest.raises(abi.PccError, match=word) as e:
            rt.cluster_frames(d_keys, 1, a["m"], a["radius2"], a["min_points"])
        assert e.value.code == abi.PCC_E_ARG
    for bad, n_frames, code, word in ((keys[::-1].copy(), 1, abi.PCC_E_ARG, "not sorted"), (keys[[0, 0, 1]], 1, abi.PCC_E_DUP, "duplicate"),
                                      (nn_ref.morton_keys(pts[:5], 2), 2, abi.PCC_E_RANGE, "frame index"),
                                      (keys, 0, abi.PCC_E_ARG, "1 .. 65535 frames")):
        with pytest.raises(abi.PccError, match=word) as e:
            rt.cluster_frames(_dev(rt, bad), n_frames, 0, 3, 1)
        assert e.value.code == code
    # after the errors the ctx is as usable as before; n = 0 launches nothing and zeroes the counts
    assert_device(device(rt, keys, 1, 0, 3, 1), replay(keys, 1, 0, 3, 1))
    assert device(rt, np.zeros(0, np.uint64), 2, 0, 3, 1)["counts"] == [[0, 0, 0, 0], [0, 0, 0, 0]]
