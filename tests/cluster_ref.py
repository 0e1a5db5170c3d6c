"""The clustering rule of include/pcc.h (pcc_cluster_frames) restated in numpy and Python integers: all pairs by brute
force for n <= 2 000, through a grid hash above that, and a sequential union-find.  It shares no code with the library.

Per frame, over its n distinct points in Morton order; only points of the same frame are neighbours.
  1 core      point i is a core point iff at least m OTHER points lie at d2 <= radius2 (m = 0: every point).
  2 edges     two core points are joined iff d2 <= radius2.
  3 roots     the connected components of the core points; a component's root is its smallest row.
  4 border    a point that is not core belongs to its nearest core point within radius2, the smallest row among
              equidistant ones; without one it is noise.
  5 pruning   size = core + border points; a component below min_points is noise as a whole.
  6 numbering the rest 0 .. K - 1 by (size descending, root row ascending); noise is -1.
"""
import numpy as np

BRUTE_MAX = 2000


def pairs(points, radius2):
    """(i, j, d2) int64 arrays of every ordered pair i != j of int [n, 3] points with d2 <= radius2"""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    n = p.shape[0]
    none = np.zeros(0, np.int64)
    if n < 2:
        return none, none, none
    if n <= BRUTE_MAX:
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        i, j = np.nonzero(d <= radius2)
        keep = i != j
        return i[keep], j[keep], d[i[keep], j[keep]]
    # grid hash: cells of edge c >= radius, so every neighbour lies in one of the 27 cells around a point's own
    c = 1
    while c * c < radius2:
        c += 1
    cell = (p - p.min(0)) // c + 1      # 1 ..: the cells around are never negative
    span = int(cell.max()) + 2
    code = (cell[:, 0] * span + cell[:, 1]) * span + cell[:, 2]
    order = np.argsort(code, kind="stable")
    sorted_code = code[order]
    out_i, out_j, out_d = [], [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                want = code + (dx * span + dy) * span + dz
                lo, hi = np.searchsorted(sorted_code, want, "left"), np.searchsorted(sorted_code, want, "right")
                cnt = hi - lo
                i = np.repeat(np.arange(n), cnt)
                at = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
                j = order[at]
                d = ((p[i] - p[j]) ** 2).sum(1)
                keep = (d <= radius2) & (i != j)
                out_i.append(i[keep]); out_j.append(j[keep]); out_d.append(d[keep])
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_d)


def components(n, i, j, d, m):
    """steps 1 .. 4 from the pairs: (core bool [n], root int [n]: the root row of every point's component, -1 without)"""
    core = np.bincount(i, minlength=n) >= m if n else np.zeros(0, bool)
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    e = core[i] & core[j] & (j < i)
    for a, b in zip(i[e].tolist(), j[e].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)      # the smallest row stays the root
    root = np.full(n, -1, np.int64)
    for x in np.flatnonzero(core).tolist():
        root[x] = find(x)
    b = ~core[i] & core[j]      # border candidates: (point, core point, d2), the best by (d2, row) first
    bi, bj, bd = i[b], j[b], d[b]
    order = np.lexsort((bj, bd, bi))
    bi, bj = bi[order], bj[order]
    first = np.ones(bi.shape[0], bool)
    first[1:] = bi[1:] != bi[:-1]
    root[bi[first]] = root[bj[first]]
    return core, root


def number(root, min_points):
    """steps 5 and 6: (labels int32 [n], sizes in label order as Python ints)"""
    n = root.shape[0]
    size = {}
    for r in root.tolist():
        if r >= 0:
            size[r] = size.get(r, 0) + 1
    alive = sorted((r for r, s in size.items() if s >= min_points), key=lambda r: (-size[r], r))
    label = {r: k for k, r in enumerate(alive)}
    labels = np.array([label.get(r, -1) for r in root.tolist()], dtype=np.int32).reshape(n)
    return labels, [size[r] for r in alive]


def cluster(points, radius2, m=0, min_points=1, _cache=None):
    """one frame's distinct points in Morton order -> dict: labels int32 [n], sizes (label order), counts (points, core
    points, clusters, noise points), core uint8 [n], root int [n] (rows of this frame, before pruning; -1 without).
    _cache: a dict that keeps the components of (radius2, m) between calls on the same points."""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    n = p.shape[0]
    key = (int(radius2), int(m))
    if _cache is not None and key in _cache:
        core, root = _cache[key]
    else:
        pk = ("pairs", int(radius2))
        if _cache is not None and pk in _cache:
            i, j, d = _cache[pk]
        else:
            i, j, d = pairs(p, int(radius2))
            if _cache is not None:
                _cache[pk] = (i, j, d)
        core, root = components(n, i, j, d, int(m))
        if _cache is not None:
            _cache[key] = (core, root)
    labels, sizes = number(root, int(min_points))
    return {"labels": labels, "sizes": sizes, "counts": (n, int(core.sum()), len(sizes), int((labels < 0).sum())),
            "core": core.astype(np.uint8), "root": root}


def cluster_rows(rows, radius2, m=0, min_points=1):
    """the label of every input row of one frame (int [n, 3], duplicates allowed, any order): that of its distinct point
    -> (labels int32 [n], the frame's `cluster` dict)"""
    import nn_ref
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    distinct = nn_ref.morton_sorted_unique(rows)
    got = cluster(distinct, radius2, m, min_points)
    label = {tuple(p): int(v) for p, v in zip(distinct.tolist(), got["labels"])}
    return np.array([label[tuple(p)] for p in rows.tolist()], dtype=np.int32).reshape(rows.shape[0]), got
