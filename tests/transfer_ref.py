"""The attribute-transfer rule of include/pcc.h (pcc_attr_transfer_frames) restated in numpy, on nn_ref's brute-force
nearest neighbours.  All sums are int64.

For a frame: the source S is a multiset of lattice points with one value row each, the target T distinct lattice points in
Morton order.  b(s) = the nearest target row of source row s, f(t) = the nearest row among the DISTINCT source points in
Morton order of target t, both with ties to the smallest row.  cnt(t) = |{s : b(s) = t}|;
out[t] = (sum of v[s] over b(s) = t + cnt // 2) // cnt where cnt > 0, else the merged value of distinct source point
f(t) — the same rounded mean over its duplicate rows — and 0 with cnt = 0 where the frame has no source.
"""
import numpy as np

import nn_ref


def merged(points, values):
    """(the distinct points in Morton order int64 [n_u, 3], their merged values int64 [n_u, c]) of a source side: the
    rounded mean (sum + cnt // 2) // cnt over the rows of every point, compress's rule for duplicate points"""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    v = np.asarray(values).astype(np.int64)
    v = v.reshape(p.shape[0], v.shape[1] if v.ndim > 1 else 1)
    _, first, inverse = np.unique(nn_ref.morton_keys(p), return_index=True, return_inverse=True)
    sums = np.zeros((first.shape[0], v.shape[1]), np.int64)
    np.add.at(sums, inverse.reshape(-1), v)
    cnt = np.bincount(inverse.reshape(-1), minlength=first.shape[0]).astype(np.int64)[:, None]
    return p[first], (sums + cnt // 2) // np.maximum(cnt, 1)


def transfer(src_points, src_values, targets):
    """(out [n_t, c] in the values' dtype, cnt uint32 [n_t]) for int [n_s, 3] source rows as they come with their values
    [n_s] or [n_s, c], and int [n_t, 3] targets, distinct and in Morton order"""
    s = np.asarray(src_points, dtype=np.int64).reshape(-1, 3)
    t = np.asarray(targets, dtype=np.int64).reshape(-1, 3)
    values = np.asarray(src_values)
    v = values.astype(np.int64).reshape(s.shape[0], values.shape[1] if values.ndim > 1 else 1)
    assert np.all(np.diff(nn_ref.morton_keys(t).astype(object)) > 0), "targets: distinct and Morton-ordered"
    if s.shape[0] == 0 or t.shape[0] == 0:
        return np.zeros((t.shape[0], v.shape[1]), values.dtype), np.zeros(t.shape[0], np.uint32)
    _, b = nn_ref.nn(s, t)
    distinct, mv = merged(s, v)
    _, f = nn_ref.nn(t, distinct)
    sums = np.zeros((t.shape[0], v.shape[1]), np.int64)
    np.add.at(sums, b, v)
    cnt = np.bincount(b, minlength=t.shape[0]).astype(np.int64)[:, None]
    out = np.where(cnt > 0, (sums + cnt // 2) // np.maximum(cnt, 1), mv[f])
    return out.astype(values.dtype), cnt[:, 0].astype(np.uint32)


def transfer_rows(src_points, src_values, target_rows):
    """what GeometryCodec.transfer returns for one frame: target rows in any order and with duplicates, every row given
    the value (and count) of its point; [n_to] for 1-D values"""
    values = np.asarray(src_values)
    rows = np.asarray(target_rows, dtype=np.int64).reshape(-1, 3)
    t = nn_ref.morton_sorted_unique(rows)
    out, cnt = transfer(src_points, values, t)
    at = np.searchsorted(nn_ref.morton_keys(t), nn_ref.morton_keys(rows))
    out, cnt = out[at], cnt[at]
    return (out[:, 0] if values.ndim == 1 else out), cnt


def hand_worked():
    """the stream that tests/test_geometry_transfer.py works by hand, on the x axis (Morton order is x order there):
    (source rows [6, 3] as they come, values uint8 [6], targets [5, 3], out [5], cnt [5])"""
    xs, vs = [39, 21, 3, 0, 6, 21], [50, 7, 1, 2, 100, 10]
    line = lambda x: np.array([[v, 0, 0] for v in x], dtype=np.int64)      # noqa: E731
    return line(xs), np.array(vs, np.uint8), line([1, 5, 20, 30, 40]), np.array([2, 100, 9, 9, 50], np.uint8), \
        np.array([2, 1, 2, 0, 1], np.uint32)


def transfer_frames(src_frames, value_frames, target_frames):
    """per-frame lists in -> (values per frame, counts per frame), each frame by transfer_rows"""
    got = [transfer_rows(s, v, t) for s, v, t in zip(src_frames, value_frames, target_frames)]
    return [g[0] for g in got], [g[1] for g in got]
