"""A second statement of attribute blob versions 28 and 31 (the rule in include/pcc.h and in csrc/attr_blob.h's header:
the bounded-error forms of versions 25 and 26), written from that description in numpy on top of tests/attr_nbr_ref.py
(candidates, weights, predictor), tests/attr_nl_ref.py (the quantiser, the coder, version 7's layout) and
tests/attr_cross_ref.py (the cross rule).  The closed loop runs size by size, 16 down to 0, over all points of a size
at once: a point's candidates were all introduced at larger sizes, so their decoded values stand.  Not a port of the
kernels.

    closed_loop(v, s, idx, w, e, mask)       -> (j [n, c], v^ [n, c] clamped), both by Morton index
    encode(points, values, bpv, e, bias=32768, cross=None) -> blob: version 28, or 31 under a mask
    decode(blob_or_prefix, cells, lod=0)     -> (values int64 [m, c], bpv): cells int [m, 3] = the distinct points >> lod
                                                (any order); row j belongs to the j-th cell in Morton order
    lod_info(blob_or_prefix, lod)            -> (bytes, values): version 7's formula
    info(blob)                               -> attr_nl_ref.info's dict with "predictor" and, for 31, "cross_channel"
encode takes layout=(S, n_chunks) and p0=; decode and lod_info take any_layout=True.
"""
import struct

import numpy as np

import attr2_ref
import attr_nbr_ref
import attr_nl_ref
from attr_cross_ref import forward, inverse, mask_of
from attr_ref import HEAD, _as2d

VERSION, VERSION_CROSS = 28, 31


def closed_loop(v, s, idx, w, e, mask):
    q = 2 * e + 1
    j = np.zeros_like(v)
    vh = np.zeros_like(v)
    for size in range(16, -1, -1):
        at = np.nonzero(s == size)[0]
        p = attr_nbr_ref.predict(vh, idx[at], w[at])                       # 0 for point 0: it has no candidate
        j[at] = attr_nl_ref.quantise(v[at] - p, e)
        vh[at] = np.clip(p + j[at] * q, 0, mask)
    return j, vh


def encode(points, values, bpv, e, bias=32768, cross=None, layout=None, p0=None):
    v = _as2d(values)
    n, c = v.shape
    m = mask_of(cross, c)
    attr_nl_ref._check_e(e, bpv)
    slod = 15 - int(bias).bit_length() + 1
    assert bias == 32768 >> slod
    assert n == 0 or (v.min() >= 0 and v.max() < 1 << (8 * bpv))
    head = bytes([ord("A"), VERSION_CROSS if m else VERSION, bpv | (slod << 4), c | (m << 4)]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    keys, srt, order, s, idx, w = attr_nbr_ref.neighbours(points, bias)
    v = v[srt]
    j, vh = closed_loop(v, s, idx, w, e, (1 << (8 * bpv)) - 1)
    assert np.abs(v - vh).max() <= e
    r = j[order]                                                           # indices in introduction order
    body = struct.pack("<I", e) + struct.pack("<16I", *[int((s >= k).sum()) for k in range(16)])
    body += attr_nl_ref._code(forward(r, m, bpv) if m else r, bpv, layout, p0)
    return head + struct.pack("<I", len(body)) + body


def _v7_head(blob):
    """the blob (or prefix) under version 7's head: the same layout, the mask taken out of byte 3 -> (blob, m)"""
    assert len(blob) >= HEAD and blob[0] == ord("A") and blob[1] in (VERSION, VERSION_CROSS), "not an attribute blob of version 28 / 31"
    c, m = (blob[3] & 15, blob[3] >> 4) if blob[1] == VERSION_CROSS else (blob[3], 0)
    assert 1 <= c <= 4 and (blob[1] == VERSION or 0 < m < 1 << (c - 1)), "mask %d with %d channels" % (m, c)
    return bytes([blob[0], 7, blob[2], c]) + bytes(blob[4:]), m


def info(blob):
    b7, m = _v7_head(blob)
    i = dict(attr_nl_ref.info(b7), version=blob[1], predictor="neighbours")
    if blob[1] == VERSION_CROSS:
        i["cross_channel"] = tuple(ch for ch in range(1, 4) if m >> (ch - 1) & 1)
    return i


def lod_info(blob, lod, any_layout=False):
    return attr_nl_ref.lod_info(_v7_head(blob)[0], lod, any_layout)


def decode(blob, cells, lod=0, any_layout=False):
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    b7, m = _v7_head(blob)
    b2, e = attr_nl_ref._lossless_shape(b7)
    bpv, c, n, h = attr2_ref._header(b2, any_layout)
    k = cells.shape[0]
    if n == 0:
        assert k == 0
        return np.zeros((0, c), np.int64), bpv
    assert k == h[0][lod], "the blob has %d values at lod %d, the geometry %d cells" % (h[0][lod], lod, k)
    assert len(b2) >= attr2_ref.lod_info(b2, lod, any_layout)[0], "truncated"
    assert h[5] + lod <= 15
    x, _ = attr2_ref._residuals(b2, k, any_layout)                          # signed, as the binarisation holds them
    j = inverse(x, m, bpv) if m else x
    keys, srt, order, s, idx, w = attr_nbr_ref.neighbours(cells, 32768 >> (h[5] + lod))
    assert [int((s >= t).sum()) for t in range(16 - lod)] == list(h[0][lod:]), "the cells do not give the header's counts"
    mask, q = (1 << (8 * bpv)) - 1, 2 * e + 1
    jm = np.zeros((k, c), np.int64)
    jm[order] = j                                                           # index of every Morton index
    val = np.zeros((k, c), np.int64)
    for size in range(16, -1, -1):                                          # a size's candidates are all coarser: done
        at = np.nonzero(s == size)[0]
        y = attr_nbr_ref.predict(val, idx[at], w[at]) + jm[at] * q
        assert (y >= -e).all() and (y <= mask + e).all(), "a reconstruction no encoder produces"
        val[at] = np.clip(y, 0, mask)
    return val, bpv
