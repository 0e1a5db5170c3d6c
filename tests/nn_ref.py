"""The nearest-neighbour rule of include/pcc.h (pcc_nn_frames) restated in numpy: brute force over all pairs, int64.

For a frame: the queries Q are a multiset of lattice points, the reference R distinct lattice points in Morton order.
d2(q) = min over r of |q - r|^2 as an integer, row(q) = the smallest row among the minimisers, rows counted over the
whole call's reference (all frames concatenated in frame order, which is the order of the call's sorted keys).  Per
frame: count = |Q_f|, sum and max of d2.  Queries of a frame without a reference: d2 = 2^64 - 1, row = -1, statistics 0.
"""
import numpy as np

NO_DIST = (1 << 64) - 1


def _spread3(v):
    x = v.astype(np.uint64) & np.uint64(0xFFFF)
    x = (x | (x << np.uint64(16))) & np.uint64(0x0000FF0000FF)
    x = (x | (x << np.uint64(8))) & np.uint64(0x00F00F00F00F)
    x = (x | (x << np.uint64(4))) & np.uint64(0x0C30C30C30C3)
    x = (x | (x << np.uint64(2))) & np.uint64(0x249249249249)
    return x


def morton_keys(points, frame=0):
    """uint64 keys of int [n, 3] points: frame << 48 | x bits at 3i + 2, y at 3i + 1, z at 3i, coordinates biased by 32768"""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3) + 32768
    assert ((p >= 0) & (p <= 65535)).all()
    return (np.uint64(frame) << np.uint64(48)) | (_spread3(p[:, 0]) << np.uint64(2)) | (_spread3(p[:, 1]) << np.uint64(1)) | _spread3(p[:, 2])


def morton_sorted_unique(points):
    """the distinct rows of int [n, 3] points in Morton order (what a reference side is)"""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    _, first = np.unique(morton_keys(p), return_index=True)
    return p[first]


def nn(queries, reference, chunk=2048):
    """(d2 uint64 [n_q], row int64 [n_q]) of int [n_q, 3] queries among the rows of int [n_r, 3] reference, as they
    come: the first row among the minimisers (np.argmin), so Morton-ordered rows give the rule's tie-break"""
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    r = np.asarray(reference, dtype=np.int64).reshape(-1, 3)
    if r.shape[0] == 0:
        return np.full(q.shape[0], NO_DIST, np.uint64), np.full(q.shape[0], -1, np.int64)
    d2 = np.empty(q.shape[0], np.uint64)
    row = np.empty(q.shape[0], np.int64)
    for a in range(0, q.shape[0], chunk):
        d = ((q[a:a + chunk, None, :] - r[None, :, :]) ** 2).sum(-1)      # at most 3 * 65535^2 < 2^63
        j = d.argmin(1)
        row[a:a + chunk] = j
        d2[a:a + chunk] = d[np.arange(j.shape[0]), j].astype(np.uint64)
    return d2, row


def nn_frames(query_frames, reference_frames):
    """per-frame lists in, the call's results out: (d2 per frame, row per frame counted over the whole call's reference,
    stats int [n_frames, 3] of Python ints: count, sum, max).  reference_frames[f] must be distinct and Morton-ordered."""
    d2s, rows, stats, first = [], [], [], 0
    for q, r in zip(query_frames, reference_frames):
        d2, row = nn(q, r)
        n_r = np.asarray(r).reshape(-1, 3).shape[0]
        if n_r:
            stats.append([int(d2.shape[0]), int(sum(int(v) for v in d2)), int(max([int(v) for v in d2], default=0))])
            row = row + first
        else:
            stats.append([0, 0, 0])
        d2s.append(d2)
        rows.append(row)
        first += n_r
    return d2s, rows, stats


def d1(a, b, peak=None):
    """{"mse_ab", "mse_ba", "max_ab", "max_ba", "d1_psnr"} of two point sets under the rule (duplicates of the query side
    count; the reference side is made distinct): mse = sum / count in float64, the PSNR formula of metrics.d1_psnr"""
    a = np.asarray(a, dtype=np.int64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.int64).reshape(-1, 3)
    out = {}
    for name, q, r in (("ab", a, b), ("ba", b, a)):
        d2, _ = nn(q, morton_sorted_unique(r))
        s = sum(int(v) for v in d2)
        out["mse_" + name] = float(s) / float(q.shape[0]) if q.shape[0] else 0.0
        out["max_" + name] = max([int(v) for v in d2], default=0)
    m = max(out["mse_ab"], out["mse_ba"])
    out["d1_psnr"] = None if peak is None else (float("inf") if m == 0.0 else float(10.0 * np.log10(3.0 * float(peak) ** 2 / m)))
    return out


def attr_mse(a_points, a_values, b_points, b_values):
    """per channel, the mean over the rows of a of (a_value - b_value[nearest row of b])^2, b distinct; float64 list"""
    a_points = np.asarray(a_points, dtype=np.int64).reshape(-1, 3)
    b_points = np.asarray(b_points, dtype=np.int64).reshape(-1, 3)
    order = np.argsort(morton_keys(b_points), kind="stable")
    _, row = nn(a_points, b_points[order])
    av = np.asarray(a_values).astype(np.int64).reshape(a_points.shape[0], -1)
    bv = np.asarray(b_values).astype(np.int64).reshape(b_points.shape[0], -1)[order][row]
    sse = ((av - bv) ** 2).sum(0)
    return [float(int(s)) / float(a_points.shape[0]) for s in sse]
