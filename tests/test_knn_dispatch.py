"""The list capacities of the neighbour calls (csrc/knn.hip: knn_with_cap maps a list of k, or of min_neighbours + 1,
entries to the capacity 8, 16 or 32) at both sides of every boundary, for each call that goes through the one
dispatcher: k in 3, 8 | 9, 16 | 17, 32 and min_neighbours in 1, 7 | 8, 15 | 16, 31.

One call of two frames: 40 distinct points of a 12^3 box, more than the largest list, so the walk runs; and 5 points,
fewer than every list above 3, so the seed is the whole frame.  Everything is an integer and held to equality.

No GPU: the host replays against the restatements, for the values the other files leave out — tests/
test_geometry_normals.py replays k = 3, 8, 16, 32, tests/test_geometry_filter.py the scores at all six k and the radius
rule at min_neighbours = 1, 7, 8, 31, tests/test_geometry_cluster.py min_neighbours = 1, 31.  gpu: the kernels against
the replays at every value.
"""
import functools

import numpy as np
import pytest

import cluster_ref
import nn_ref
import normals_ref
import outlier_ref
from conftest import pkg, random_cloud

KS = (3, 8, 9, 16, 17, 32)
MS = (1, 7, 8, 15, 16, 31)
# the radius rule: a radius at which the large frame has kept and dropped points (test_the_radii_split_the_large_frame)
RADIUS2 = {1: 6, 7: 30, 8: 30, 15: 50, 16: 50, 31: 80}
MIN_POINTS = 2


@functools.lru_cache(maxsize=None)
def call():
    """(frames: the Morton-ordered distinct points of both, keys of the call)"""
    rng = np.random.default_rng(20261021)
    frames = [nn_ref.morton_sorted_unique(random_cloud(rng, n, extent=12, lo=-6)[:, 1:]) for n in (40, 5)]
    assert [f.shape[0] for f in frames] == [40, 5]
    return frames, np.concatenate([nn_ref.morton_keys(f, i) for i, f in enumerate(frames)])


@functools.lru_cache(maxsize=None)
def knn_replay(k):
    keys = call()[1]
    n = keys.shape[0]
    rows, d2 = np.zeros((n, k), np.int32), np.zeros((n, k), np.uint64)
    rc = pkg("_abi").lib().pcc_knn_replay_host(keys.ctypes.data, n, k, rows.ctypes.data, d2.ctypes.data, None, None, None)
    assert rc == 0
    return rows, d2


@functools.lru_cache(maxsize=None)
def outlier_replay(k=3, m=1):
    return pkg("runtime").Runtime.outlier_replay_host(call()[1], 2, k=k, min_neighbours=m, radius2=RADIUS2[m])


@functools.lru_cache(maxsize=None)
def cluster_replay(m):
    return pkg("runtime").Runtime.cluster_replay_host(call()[1], 2, m, RADIUS2[m], MIN_POINTS)


# ------------------------------------------------------------------ the replays against the restatements
@pytest.mark.parametrize("m", MS)
def test_the_radii_split_the_large_frame(m):
    kept = int(outlier_ref.radius(call()[0][0], m, RADIUS2[m]).sum())
    assert 0 < kept < 40


@pytest.mark.parametrize("k", (9, 17))
def test_knn_replay_at_the_capacity_boundaries(k):
    want_rows, want_d2, _ = normals_ref.knn_frames(call()[0], k)
    rows, d2 = knn_replay(k)
    assert np.array_equal(rows, want_rows) and np.array_equal(d2, want_d2)
    assert np.all(rows[40:, 5:] == -1) and np.all(rows[40:, :5] >= 40)      # the small frame: its 5 points, then nothing


@pytest.mark.parametrize("m", (15, 16))
def test_radius_replay_at_the_capacity_boundaries(m):
    got = outlier_replay(m=m)
    want = np.concatenate([outlier_ref.radius(f, m, RADIUS2[m]) for f in call()[0]]).astype(np.uint8)
    assert np.array_equal(got["keep_unbounded"], want)
    assert np.array_equal(got["keep_radius"], got["keep_unbounded"])
    assert not want[40:].any()      # 5 points: nobody has 15 neighbours


@pytest.mark.parametrize("m", (7, 8, 15, 16))
def test_cluster_replay_at_the_capacity_boundaries(m):
    got = cluster_replay(m)
    want = [cluster_ref.cluster(f, RADIUS2[m], m, MIN_POINTS) for f in call()[0]]
    assert np.array_equal(got["labels"], np.concatenate([w["labels"] for w in want]))
    assert np.array_equal(got["core"], np.concatenate([w["core"] for w in want]))
    assert got["counts"] == [list(w["counts"]) for w in want]
    for first, w in zip((0, 40), want):
        assert got["sizes"][first:first + len(w["sizes"])].tolist() == list(w["sizes"])


# ------------------------------------------------------------------ the kernels against the replays
def _dev(rt, keys):
    import torch
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(rt.device)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_knn_and_scores_on_the_device_at_every_capacity(rt, k):
    keys = _dev(rt, call()[1])
    rows, d2, _, _ = rt.knn_frames(keys, 2, k, want_rows=True, want_dist=True, want_normals=False)
    scores, sums = rt.outlier_scores_frames(keys, 2, k)      # synchronises
    want_rows, want_d2 = knn_replay(k)
    assert np.array_equal(rows.cpu().numpy(), want_rows)
    assert np.array_equal(d2.cpu().numpy().view(np.uint64), want_d2)
    want = outlier_replay(k=k)
    assert np.array_equal(scores.cpu().numpy().view(np.uint64), want["scores"])
    assert sums == want["sums"]


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
def test_radius_rule_and_clusters_on_the_device_at_every_capacity(rt, m):
    keys = _dev(rt, call()[1])
    keep, counts = rt.outlier_radius_frames(keys, 2, m, RADIUS2[m])
    labels, sizes, ccounts = rt.cluster_frames(keys, 2, m, RADIUS2[m], MIN_POINTS)
    rt.sync()
    want = outlier_replay(m=m)["keep_radius"]
    assert np.array_equal(keep.cpu().numpy(), want)
    assert counts.cpu().tolist() == [[40, int(want[:40].sum())], [5, int(want[40:].sum())]]
    got = cluster_replay(m)
    assert np.array_equal(labels.cpu().numpy(), got["labels"])
    assert np.array_equal(sizes.cpu().numpy().view(np.uint32), got["sizes"])
    assert ccounts.cpu().tolist() == got["counts"]
