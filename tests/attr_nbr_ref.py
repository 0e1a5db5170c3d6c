"""A second statement of attribute blob versions 25 and 26 (the rule in include/pcc.h and in csrc/attr_blob.h's header:
lossless values predicted from up to three representatives of the coarser cells around a point), written from that
description in numpy on top of tests/attr2_ref.py (keys, introduction order, the reader of the lanes) and
tests/attr_nl_ref.py's coder, which codes what it is handed under version 2's contexts.  The candidates of all points
come from 27 searchsorted calls, one per offset, the choice from one sort per point over (d, Morton index); the decoder
rebuilds the values size by size, 16 down to 0, since a point's candidates were all introduced at larger sizes.  Not a
port of the kernels.

    neighbours(points, bias, tie=1)          -> (keys, order, s, idx [n, 3], w [n, 3]) of distinct points (any order):
                                                sorted keys, introduction order, sizes, and per Morton index the chosen
                                                candidates' Morton indexes (-1: none) and weights (0: none); tie = -1
                                                reverses the tie-break on the Morton index (tests only)
    predict(v, idx, w)                       -> p int64 [n, c] of rows whose candidates' values stand in v
    encode(points, values, bpv, bias=32768, cross=None) -> blob: version 25, or 26 under a mask (attr_cross_ref.mask_of)
    decode(blob_or_prefix, cells, lod=0)     -> (values int64 [m, c], bpv): cells int [m, 3] = the distinct points >> lod
                                                (any order); row j belongs to the j-th cell in Morton order
    lod_info(blob_or_prefix, lod)            -> (bytes, values): version 2's formula
encode takes layout=(S, n_chunks), p0= and tie=; decode and lod_info take any_layout=True, decode tie=.
"""
import struct

import numpy as np

import attr2_ref
import attr_nl_ref
from attr_cross_ref import _wrap, forward, inverse, mask_of
from attr_ref import HEAD, _as2d

VERSION, VERSION_CROSS = 25, 26
OFFSETS = [(ox, oy, oz) for ox in (-1, 0, 1) for oy in (-1, 0, 1) for oz in (-1, 0, 1)]


def neighbours(points, bias=32768, tie=1):
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    keys = attr2_ref.keys_of(pts, bias)
    srt = np.argsort(keys, kind="stable")
    keys, P = keys[srt], pts[srt] + bias
    n = keys.shape[0]
    s, order, _ = attr2_ref.intro(keys)
    side = 2 * bias                                                        # the lattice [0, side) per axis
    idx = np.full((n, 3), -1, np.int64)
    w = np.zeros((n, 3), np.int64)
    if n < 2:
        return keys, srt, order, s, idx, w
    sh = np.minimum(s, 15)                                                 # point 0 (s = 16) has no candidates: masked below
    u = P >> sh[:, None]
    C = P >> (sh[:, None] + 1)
    big = np.int64(1) << 62
    rank = np.full((n, 27), big, np.int64)                                 # d << 32 | Morton index, or none
    for t, o in enumerate(OFFSETS):
        q = C + np.asarray(o, np.int64)
        org = q << (sh[:, None] + 1)                                       # the cell's origin
        inside = ((q >= 0) & (org < side)).all(1)
        qq = np.where(inside[:, None], q, 0)
        ck = (attr2_ref._spread3(qq[:, 0]) << np.uint64(2)) | (attr2_ref._spread3(qq[:, 1]) << np.uint64(1)) | attr2_ref._spread3(qq[:, 2])
        bits = (3 * (sh + 1)).astype(np.uint64)
        j = np.searchsorted(keys, ck << bits)                              # the frame's Morton-first point not in front of the cell
        jj = np.minimum(j, n - 1)
        hit = inside & (j < n) & ((keys[jj] >> bits) == ck)
        diff = (P[jj] >> sh[:, None]) - u
        d = (diff * diff).sum(1)
        assert (d[hit & (s < 16)] >= 1).all() and (d[hit] <= 27).all()
        rank[:, t] = np.where(hit, (d << 32) | (jj if tie > 0 else n - 1 - jj), big)
    rank[0] = big
    rank = np.sort(rank, axis=1)[:, :3]
    have = rank < big
    j3 = rank & 0xFFFFFFFF
    idx = np.where(have, j3 if tie > 0 else n - 1 - j3, -1)
    w = np.where(have, 65536 // np.maximum(rank >> 32, 1), 0)
    assert have[1:, 0].all(), "first(i) is always there"
    assert (s[np.maximum(idx, 0)] > s[:, None])[have].all(), "a candidate was introduced at a larger size"
    return keys, srt, order, s, idx, w


def predict(v, idx, w):
    """floor((2 sum w v_j + sum w) / (2 sum w)) per channel; rows without a candidate: 0"""
    sw = w.sum(1)
    acc = (w[:, :, None] * v[np.maximum(idx, 0)]).sum(1)
    return np.where(sw[:, None] > 0, (2 * acc + sw[:, None]) // np.maximum(2 * sw[:, None], 1), 0)


def encode(points, values, bpv, bias=32768, cross=None, layout=None, p0=None, tie=1):
    v = _as2d(values)
    n, c = v.shape
    m = mask_of(cross, c)
    slod = 15 - int(bias).bit_length() + 1
    assert bias == 32768 >> slod
    assert n == 0 or (v.min() >= 0 and v.max() < 1 << (8 * bpv))
    head = bytes([ord("A"), VERSION_CROSS if m else VERSION, bpv | (slod << 4), c | (m << 4)]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    keys, srt, order, s, idx, w = neighbours(points, bias, tie)
    v = v[srt]
    r = _wrap(v - predict(v, idx, w), bpv)[order]                          # residuals in introduction order
    body = struct.pack("<16I", *[int((s >= k).sum()) for k in range(16)])
    body += attr_nl_ref._code(forward(r, m, bpv) if m else r, bpv, layout, p0)
    return head + struct.pack("<I", len(body)) + body


def _v2_head(blob):
    """the blob (or prefix) under version 2's head: the same layout, the mask taken out of byte 3 -> (blob, m)"""
    assert len(blob) >= HEAD and blob[0] == ord("A") and blob[1] in (VERSION, VERSION_CROSS), "not an attribute blob of version 25 / 26"
    c, m = (blob[3] & 15, blob[3] >> 4) if blob[1] == VERSION_CROSS else (blob[3], 0)
    assert 1 <= c <= 4 and (blob[1] == VERSION or 0 < m < 1 << (c - 1)), "mask %d with %d channels" % (m, c)
    return bytes([blob[0], 2, blob[2], c]) + bytes(blob[4:]), m


def lod_info(blob, lod, any_layout=False):
    return attr2_ref.lod_info(_v2_head(blob)[0], lod, any_layout)


def residuals(blob, m_values, any_layout=False):
    """the first m_values residuals of the introduction order, the cross rule undone"""
    b2, m = _v2_head(blob)
    x, bpv = attr2_ref._residuals(b2, m_values, any_layout)
    return (inverse(x, m, bpv) if m else x), bpv


def decode(blob, cells, lod=0, any_layout=False, tie=1):
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    b2, _ = _v2_head(blob)
    bpv, c, n, h = attr2_ref._header(b2, any_layout)
    k = cells.shape[0]
    if n == 0:
        assert k == 0
        return np.zeros((0, c), np.int64), bpv
    assert k == h[0][lod], "the blob has %d values at lod %d, the geometry %d cells" % (h[0][lod], lod, k)
    assert len(b2) >= attr2_ref.lod_info(b2, lod, any_layout)[0], "truncated"
    assert h[5] + lod <= 15
    r, _ = residuals(blob, k, any_layout)
    keys, srt, order, s, idx, w = neighbours(cells, 32768 >> (h[5] + lod), tie)
    assert [int((s >= j).sum()) for j in range(16 - lod)] == list(h[0][lod:]), "the cells do not give the header's counts"
    mask = (1 << (8 * bpv)) - 1
    res = np.zeros((k, c), np.int64)
    res[order] = r                                                          # residual of every Morton index
    val = np.zeros((k, c), np.int64)
    for size in range(16, -1, -1):                                          # a size's candidates are all coarser: done
        at = np.nonzero(s == size)[0]
        val[at] = (predict(val, idx[at], w[at]) + res[at]) & mask
    return val, bpv
