"""The outlier rules of include/pcc.h (pcc_outlier_scores_frames, pcc_outlier_mask_frames, pcc_outlier_radius_frames)
restated in numpy and Python integers, on normals_ref.knn's brute-force neighbours.

Per frame, over its n distinct points in Morton order; only points of the same frame are neighbours.
Statistical: q_i = sum over the k_eff = min(k, n) neighbours (the point itself included, at 0) of floor(16 sqrt(d2)),
each term the integer square root of d2 << 8; S1 = sum q, S2 = sum q^2; R = rint(256 std_ratio); T the largest integer t
with n t <= S1 or 65536 (n - 1) (n t - S1)^2 <= R^2 n (n S2 - S1^2), 2^64 - 1 for n < 2; keep iff q_i <= T.
Radius: keep iff at least m other points of the frame lie at d2 <= radius2.
"""
import numpy as np

import normals_ref

KEEP_ALL = (1 << 64) - 1


def isqrt(x):
    """floor(sqrt(x)) of a non-negative Python integer, by bisection on integers alone"""
    lo, hi = 0, 1
    while hi * hi <= x:
        hi *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid * mid <= x:
            lo = mid
        else:
            hi = mid
    return lo


def scores(points, k):
    """q per point (a list of Python ints) of int [n, 3] distinct points in Morton order"""
    _, d2 = normals_ref.knn(points, k)
    return [sum(isqrt(int(d) << 8) for d in row if int(d) != normals_ref.NO_DIST) for row in d2]


def ratio(std_ratio):
    return int(np.rint(256.0 * std_ratio))


def admits(t, n, s1, s2, r):
    """whether t is at most mean + (r / 256) std: the rule's inequality as it stands"""
    return n * t <= s1 or 65536 * (n - 1) * (n * t - s1) ** 2 <= r * r * n * (n * s2 - s1 * s1)


def threshold(q, r):
    """T for the scores q of one frame: the largest t that `admits`, found by bisection between S1 div n (admitted:
    n t <= S1) and a bound that is not (above the largest score by more than 255 standard deviations could span)"""
    n = len(q)
    if n < 2:
        return KEEP_ALL
    s1, s2 = sum(q), sum(v * v for v in q)
    lo, hi = s1 // n, s1 // n + 1
    while admits(hi, n, s1, s2, r):
        hi = 2 * hi + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if admits(mid, n, s1, s2, r):
            lo = mid
        else:
            hi = mid
    return lo


def statistical(points, k, std_ratio):
    """-> (keep bool [n], report) of one frame's distinct points in Morton order"""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    q = scores(p, k)
    t = threshold(q, ratio(std_ratio))
    keep = np.array([v <= t for v in q], dtype=bool)
    return keep, {"points": len(q), "kept": int(keep.sum()), "k_eff": min(k, len(q)), "S1": sum(q), "S2": sum(v * v for v in q),
                  "threshold": t, "scores": q}


def radius(points, m, radius2):
    """-> keep bool [n]: at least m other points within radius2, counted over all pairs"""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    if p.shape[0] == 0:
        return np.zeros(0, bool)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return (d <= min(int(radius2), 3 * 65535 ** 2)).sum(1) - 1 >= m


def filter_rows(rows, keep_fn):
    """the verdict of every input row of one frame (int [n, 3], duplicates allowed, any order): that of its distinct
    point; keep_fn: the Morton-ordered distinct points -> keep bool"""
    import nn_ref
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    distinct = nn_ref.morton_sorted_unique(rows)
    keep = keep_fn(distinct)
    verdict = {tuple(p): bool(k) for p, k in zip(distinct.tolist(), keep)}
    return np.array([verdict[tuple(p)] for p in rows.tolist()], dtype=bool), distinct, keep
