"""The k-nearest-neighbour, scatter-matrix, normal and D2 rules of include/pcc.h (pcc_knn_frames, pcc_nn_d2_frames)
restated in numpy: brute force over all pairs, integers where the rule is in integers.

k nearest neighbours: per frame the reference is the frame's distinct points in Morton order, the queries those same
points; knn(p) = the first k_eff = min(k, n_f) rows ordered by (|r - p|^2, row) ascending — p itself first, at distance
0, and the smaller row (Morton-first) among equidistant ones; rows counted over the whole call; slots k_eff .. k - 1
hold row -1 and d2 = 2^64 - 1.
Scatter matrix: C = m sum d d^T - (sum d)(sum d)^T over the m = k_eff neighbours, d = r - p, int64: xx xy xz yy yz zz.
Normal: a unit eigenvector of C for its smallest eigenvalue (here numpy.linalg.eigh's), float32; frames with fewer
than 3 distinct points have none (zeros, C = 0); with a viewpoint n is flipped where n . (viewpoint - p) < 0.
D2: proj = ((ex nx + ey ny) + ez nz)^2 in float64 with the normal of the pair's A point; mse = sum proj / count.
"""
import math

import numpy as np

import nn_ref

NO_DIST = nn_ref.NO_DIST


def knn(points, k):
    """(rows int64 [n, k], d2 uint64 [n, k]) of int [n, 3] points in Morton order among themselves"""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    n = p.shape[0]
    rows = np.full((n, k), -1, np.int64)
    d2 = np.full((n, k), NO_DIST, np.uint64)
    if n == 0:
        return rows, d2
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]      # stable: the smaller row first among equal distances
    m = order.shape[1]
    rows[:, :m] = order
    d2[:, :m] = np.take_along_axis(d, order, 1).astype(np.uint64)
    return rows, d2


def scatter(points, rows):
    """C int64 [n, 6] (xx, xy, xz, yy, yz, zz) of the neighbourhoods `rows` (local rows, -1 = no neighbour); zeros for a
    frame of fewer than 3 points"""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    n = p.shape[0]
    out = np.zeros((n, 6), np.int64)
    if n < 3:
        return out
    have = rows >= 0
    d = (p[np.where(have, rows, 0)] - p[:, None, :]) * have[:, :, None]
    m = have.sum(1)
    s = d.sum(1)
    for c, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        out[:, c] = m * (d[:, :, i] * d[:, :, j]).sum(1) - s[:, i] * s[:, j]
    return out


def sym(c):
    """[n, 6] -> float64 [n, 3, 3]"""
    c = np.asarray(c).astype(np.float64).reshape(-1, 6)
    return c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def normals_of(c, points=None, viewpoint=None):
    """float32 [n, 3]: numpy.linalg.eigh's eigenvector of the smallest eigenvalue of every C"""
    n = np.linalg.eigh(sym(c))[1][:, :, 0].astype(np.float32)
    if viewpoint is not None:
        e = np.asarray(viewpoint, np.float64)[None, :] - np.asarray(points, np.float64)
        nd = n.astype(np.float64)
        dot = (e[:, 0] * nd[:, 0] + e[:, 1] * nd[:, 1]) + e[:, 2] * nd[:, 2]
        n = np.where((dot < 0)[:, None], -n, n)
    return n


def rayleigh_check(c, normals):
    """the check of the issue for every row: finite, | |n| - 1 | <= 1e-6, n^T C n / n^T n <= l0 + 1e-6 max(l2, 1) with
    the eigenvalues of numpy.linalg.eigvalsh in float64.  Returns the number of rows that fail."""
    a = sym(c)
    n = np.asarray(normals).astype(np.float64).reshape(-1, 3)
    lam = np.linalg.eigvalsh(a)
    nn_ = (n * n).sum(1)
    bad = ~np.isfinite(n).all(1)
    bad |= ~(np.abs(np.sqrt(nn_) - 1.0) <= 1e-6)
    with np.errstate(all="ignore"):
        q = np.einsum("ni,nij,nj->n", n, a, n) / nn_
    bad |= ~(q <= lam[:, 0] + 1e-6 * np.maximum(lam[:, 2], 1.0))
    return int(bad.sum())


def knn_frames(frames, k):
    """per-frame Morton-ordered distinct points in, the call's results out: (rows [n, k] counted over the whole call,
    d2 [n, k], C [n, 6]), the frames behind one another"""
    rows, d2s, cs, first = [], [], [], 0
    for p in frames:
        p = np.asarray(p, dtype=np.int64).reshape(-1, 3)
        r, d = knn(p, k)
        cs.append(scatter(p, r))
        rows.append(np.where(r >= 0, r + first, -1))
        d2s.append(d)
        first += p.shape[0]
    return np.concatenate(rows), np.concatenate(d2s), np.concatenate(cs)


def proj(q, r, n):
    """float64 [n]: ((q - r) . n)^2 row by row, the dot product as (ex nx + ey ny) + ez nz in float64"""
    e = (np.asarray(q, np.int64) - np.asarray(r, np.int64)).astype(np.float64)
    n = np.asarray(n, np.float32).astype(np.float64)
    d = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    return d * d


def d2(a, b, normals_a, peak=None):
    """{"d2_mse_ab", "d2_mse_ba", "d2_psnr"} and the per-row proj of both directions ("proj_ab" in the row order of a,
    "proj_ba" in the row order of b) for a duplicate-free a with one normal per row; sums by math.fsum"""
    a = np.asarray(a, dtype=np.int64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.int64).reshape(-1, 3)
    normals_a = np.asarray(normals_a, np.float32).reshape(-1, 3)
    out = {}
    rb = nn_ref.morton_sorted_unique(b)
    _, row = nn_ref.nn(a, rb)
    out["proj_ab"] = proj(a, rb[row], normals_a) if a.shape[0] else np.zeros(0)
    order = np.argsort(nn_ref.morton_keys(a), kind="stable")
    _, row = nn_ref.nn(b, a[order])
    out["proj_ba"] = proj(b, a[order][row], normals_a[order][row]) if b.shape[0] else np.zeros(0)
    for name in ("ab", "ba"):
        p = out["proj_" + name]
        out["d2_mse_" + name] = math.fsum(p.tolist()) / p.shape[0] if p.shape[0] else 0.0
    m = max(out["d2_mse_ab"], out["d2_mse_ba"])
    out["d2_psnr"] = None if peak is None else (float("inf") if m == 0.0 else float(10.0 * np.log10(3.0 * float(peak) ** 2 / m)))
    return out
