"""Seeded inputs for tests/test_capture.py: the edges of the capture pre-step (csrc/voxelize.hip, capture.py).
Every generator is cached; callers must leave what they get unchanged."""
import functools

import numpy as np

GRID = 1024 * 256          # threads of pcc_vox_valid's capped grid: rows from here on are a thread's second row


def pack(points, rng):
    """XYZRGBA float32 [n,4]: random r,g,b in the low three bytes of the 4th float"""
    n = points.shape[0]
    rgba = (rng.integers(0, 256, n, dtype=np.uint32) | (rng.integers(0, 256, n, dtype=np.uint32) << 8)
            | (rng.integers(0, 256, n, dtype=np.uint32) << 16) | (np.uint32(255) << 24))
    data = np.empty((n, 4), np.float32)
    data[:, :3] = points
    data[:, 3] = rgba.view(np.float32)
    return data


def norm32(points):
    """sqrt((x*x + y*y) + z*z), every step rounded to float32"""
    x, y, z = (np.ascontiguousarray(points[:, a], dtype=np.float32) for a in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((x * x + y * y) + z * z)


def norm64(points):
    """the same norm in double precision, not rounded to float32"""
    p = np.asarray(points[:, :3], dtype=np.float64)
    return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def voxel_means(data, depth_clip, voxel):
    """mean position of every Open3D voxel [v,3] (float64), by a route of its own (np.unique + np.add.at).
    Exact, hence independent of the order, wherever the sums are exact (lattice inputs)."""
    from oracle import capture_ref as ref
    p = data[ref.valid_mask(data, depth_clip), :3].astype(np.float64)
    idx = np.floor((p - (p.min(axis=0) - voxel * 0.5)) / voxel).astype(np.int64)
    _, inv, cnt = np.unique(idx, axis=0, return_inverse=True, return_counts=True)
    s = np.zeros((cnt.shape[0], 3))
    np.add.at(s, inv.reshape(-1), p)
    return s / cnt[:, None]


def round_half_away(q):
    return np.sign(q) * np.floor(np.abs(q) + 0.5)


# ------------------------------------------------------------------ ties
TIES_VOXEL, TIES_CLIP = 0.5, 100.0


def ties_frame():
    """8 points, x = -1.25 ... 2.25 in steps of 0.5, y the same reversed, z = 0.25; colours 10*i + (1,2,3)"""
    x = -1.25 + 0.5 * np.arange(8)
    data = np.empty((8, 4), np.float32)
    data[:, 0], data[:, 1], data[:, 2] = x, x[::-1], 0.25
    i = np.arange(8, dtype=np.uint32)
    data[:, 3] = ((10 * i + 1) | ((10 * i + 2) << 8) | ((10 * i + 3) << 16) | (np.uint32(255) << 24)).view(np.float32)
    return data


@functools.lru_cache(maxsize=None)
def lattice_cloud(n=20000, seed=11):
    """coordinates multiples of 0.25 in [-4, 4] (for voxel 0.5): every Open3D voxel boundary lies on points,
    a voxel holds two lattice values per axis, and its mean / 0.5 is on .5 whenever all its points share one"""
    rng = np.random.default_rng(seed)
    return pack(rng.integers(-16, 17, (n, 3)) * 0.25, rng)


# ------------------------------------------------------------------ dense voxels, duplicates
DENSE_VOXEL = 0.1


@functools.lru_cache(maxsize=None)
def dense_cloud(n, seed=5):
    """uniform(0, 0.2) at voxel 0.1: 27 voxels of n / 27 points each"""
    rng = np.random.default_rng(seed)
    return pack(rng.uniform(0.0, 0.2, (n, 3)), rng)


COLLISION_VOXEL = 0.02


@functools.lru_cache(maxsize=None)
def collision_cloud(n=6000, seed=9):
    """sparse random cloud: Open3D's grid starts at min_bound - voxel/2, the integer voxels are centred on
    multiples of the voxel; the shift by a third of a voxel sets the two grids apart, so neighbouring Open3D
    voxels often round to the same integer voxel"""
    rng = np.random.default_rng(seed)
    return pack(rng.uniform(-0.5, 0.5, (n, 3)) + COLLISION_VOXEL / 3, rng)


# ------------------------------------------------------------------ depth clip
CLIP = 1.4


@functools.lru_cache(maxsize=None)
def clip_rows(seed=3, per_class=1500):
    """Rows whose float32 step-by-step norm is exactly float32(1.4), one ulp below and one ulp above, found by
    a seeded search over random directions scaled to within a few ulps of the clip; among them every row of
    the search whose double-precision norm (unrounded, or rounded to float32 at the end) falls on the other
    side.  Returns (data, classes) with classes[i] in {-1, 0, +1} ulps from the clip."""
    rng = np.random.default_rng(seed)
    clip = np.float32(CLIP)
    d = rng.normal(size=(400000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= CLIP * (1.0 + rng.integers(-3, 4, (d.shape[0], 1)) * 2.0 ** -24)
    p = d.astype(np.float32)
    n32 = norm32(p)
    below, above = np.nextafter(clip, np.float32(0)), np.nextafter(clip, np.float32(2))
    cls = np.select([n32 == below, n32 == clip, n32 == above], [-1, 0, 1], 9)
    n64 = norm64(p)
    other = ((n64 <= np.float64(clip)) != (n32 <= clip)) | ((n64.astype(np.float32) <= clip) != (n32 <= clip))
    take = [np.flatnonzero(other & (cls != 9))[:per_class]]
    take += [np.flatnonzero(cls == c)[:per_class] for c in (-1, 0, 1)]
    rows = np.unique(np.concatenate(take))
    rows = rows[rng.permutation(rows.shape[0])]
    return pack(p[rows], rng), cls[rows]


# ------------------------------------------------------------------ frames longer than pcc_vox_valid's grid
VARIANTS = ("positive", "negative", "mixed", "zero")
_BOX = {   # per axis (lo, hi) of the ordinary valid rows; every corner is inside the 1.4 m clip
    "positive": ((0.2, 0.7), (0.25, 0.7), (0.3, 0.7)),
    "negative": ((-0.7, -0.2), (-0.7, -0.25), (-0.7, -0.3)),
    "mixed": ((0.2, 0.7), (-0.7, -0.2), (-0.5, 0.5)),
    "zero": ((0.01, 0.6), (0.2, 0.7), (-0.6, -0.1)),
}


@functools.lru_cache(maxsize=None)
def strided_frame(m, variant, seed=0):
    """[m,4] frame, mostly NaN rows.  Up to 3000 valid rows below row GRID and up to 2000 from GRID on; each
    axis's minimum sits in valid rows from GRID on wherever the frame has such rows (m = 2*GRID + 1: in its
    last row, a thread's third).  Rows beyond the clip or with an infinite coordinate carry values below every
    minimum, so counting one of them shows.  "zero": the minimum of x is 0.0, held by rows of both signs."""
    rng = np.random.default_rng([seed, m, VARIANTS.index(variant)])
    box = np.asarray(_BOX[variant])
    p = np.full((m, 3), np.nan, np.float32)
    lo_n = min(m, GRID)
    rows = rng.choice(lo_n, size=min(3000, max(1, lo_n * 3 // 4)), replace=False)
    if m > GRID:
        hi = GRID + rng.choice(m - GRID, size=min(m - GRID, 2000), replace=False)
        if m == 2 * GRID + 1:
            hi = np.union1d(hi, [2 * GRID])
        rows = np.concatenate([rows, hi])
    else:
        hi = rows
    p[rows] = rng.uniform(box[:, 0], box[:, 1], (rows.shape[0], 3)).astype(np.float32)
    # the minima: below the box by 0.05, each axis in a row of its own where there are three
    at = np.full(3, 2 * GRID) if m == 2 * GRID + 1 else rng.choice(hi, size=3, replace=hi.shape[0] < 3)
    for a in range(1 if variant == "zero" else 0, 3):
        p[at[a], a] = np.float32(box[a, 0] - 0.05)
    if variant == "zero":
        zr = hi[:24]
        p[zr, 0] = np.where(np.arange(zr.shape[0]) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    # rows that must not count: far ones and ones with an infinite coordinate, below every minimum
    free = np.setdiff1d(np.arange(m), rows)
    if free.shape[0]:
        far = free[rng.permutation(free.shape[0])[:400]]
        p[far[0::2]] = np.float32(-5.0)
        p[far[1::2]] = (np.float32(-np.inf), np.float32(-0.9), np.float32(-0.9))
    return pack(p, rng)
