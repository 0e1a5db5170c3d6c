"""A second statement of the transform-coded attribute blob with level-of-detail prefixes, version 22 (the rule in
include/pcc.h, the layout in csrc/attr_blob.h's header), written from that description in numpy.  It takes from
tests/attr_transform_ref.py and tests/attr_colour_ref.py what the kinds share by definition (sublevels, pairs, the
coding order, the integer root, the colour transform, the entropy stage _code) and from tests/attr2_ref.py the reader of
a prefix; the weights, the steps and both lifting passes are its own.  Not a port of the kernels.

    kcells(kappa, j, K)                       -> g int64 [m + 1]: K-cells in front of every cell of lod j (g[m] = all)
    scale(n, C)                               -> M = max(1, floor((2 n + C) / (2 C)))
    forward(keys, v, q, bpv, K)               -> x int64 [n, c] by Morton index; q one step per channel
    inverse(kappa, x, q, bpv, K, j, n, C, clamp=True)
                                              -> node values int64 [m, c] of the cells kappa = key >> 3 j of lod j
    stopped(keys, x, q, bpv, K, j)            -> the full inverse run over sublevels 47 .. 3 j only: the values it holds
                                                 at the first leaf of every cell of lod j, not clamped
    encode(points, values, bpv, q, K, colour=0, bias=32768)  -> blob
    decode(blob_or_prefix, cells, lod=0)      -> (values int64 [m, c], bpv): cells int [m, 3] the distinct points >> lod
    lod_info(blob_or_prefix, lod)             -> (bytes, values)
    info(blob)                                -> dict(version, bpv, channels, points, qstep (a tuple), colour,
                                                 max_error, scalable, scalable_to, lod)
"""
import struct

import numpy as np

import attr2_ref
from attr_colour_ref import _check_colour, _steps, colour_forward, colour_inverse
from attr_ref import HEAD, _as2d
from attr_transform_ref import TOP, _code, _isqrt, _slod, _sorted, order_of, pairs, sublevels

VERSION = 22


def _check_k(K, slod):
    assert isinstance(K, (int, np.integer)) and not isinstance(K, bool) and 1 <= K and slod + K <= 15, \
        "scalable_to %r with a sender's lod of %d" % (K, slod)


def kcells(kappa, j, K):
    b = sublevels(kappa)
    first = (b + 3 * j >= 3 * K).astype(np.int64)
    first[0] = 1
    return np.concatenate([[0], np.cumsum(first)])


def scale(n, C):
    return max(1, (2 * n + C) // (2 * C))


def _step_w(q, ca, cb, M):
    """[pairs, c]: s[ch] = max(2, isqrt(floor(q[ch]^2 w / (ca cb M))))"""
    ca, cb = np.asarray(ca, np.int64)[:, None], np.asarray(cb, np.int64)[:, None]
    v = (q * q)[None, :] * (ca + cb) // (ca * cb * M)
    return np.maximum(2, _isqrt(v.reshape(-1)).reshape(v.shape))


def _step_l(q, t):
    """[1, c]: s[ch] = max(2, isqrt(floor(2 q[ch]^2 / 2^floor(2 t / 3))))"""
    return np.maximum(2, _isqrt((2 * q * q) >> ((2 * t) // 3)))[None, :]


def forward(keys, v, q, bpv, K):
    H = 1 << (8 * bpv - 1)
    val = np.array(v, np.int64)
    n = val.shape[0]
    q = _steps(q, val.shape[1], bpv)
    x = np.zeros_like(val)
    b = sublevels(keys)
    g = kcells(keys, 0, K)
    M = scale(n, int(g[n]))
    for t in range(TOP):
        at, lo, wa, wb = pairs(keys, b, t)
        if at.shape[0] == 0:
            continue
        h = val[at] - val[lo]
        if t >= 3 * K:
            ca, cb = g[at] - g[lo], g[at + wb] - g[at]
            val[lo] += (cb[:, None] * h) // (ca + cb)[:, None]
            s = _step_w(q, ca, cb, M)
        else:
            val[lo] += h >> 1
            s = _step_l(q, t)
        x[at] = np.sign(h) * np.minimum((np.abs(h) + s // 2) // s, H - 1)
    x[0] = val[0] - H
    return x


def inverse(kappa, x, q, bpv, K, j, n, C, clamp=True):
    H = 1 << (8 * bpv - 1)
    x = np.asarray(x, np.int64)
    q = _steps(q, x.shape[1], bpv)
    val = np.zeros_like(x)
    val[0] = x[0] + H
    b = sublevels(kappa)
    g = kcells(kappa, j, K)
    assert int(g[-1]) == C, "the cells give %d cells of lod %d, the header %d" % (int(g[-1]), K, C)
    M = scale(n, C)
    for tp in range(TOP - 1 - 3 * j, -1, -1):
        at, lo, wa, wb = pairs(kappa, b, tp)
        if at.shape[0] == 0:
            continue
        t = tp + 3 * j
        if t >= 3 * K:
            ca, cb = g[at] - g[lo], g[at + wb] - g[at]
            hh = x[at] * _step_w(q, ca, cb, M)
            va = val[lo] - (cb[:, None] * hh) // (ca + cb)[:, None]
        else:
            hh = x[at] * _step_l(q, t)
            va = val[lo] - (hh >> 1)
        val[lo] = va
        val[at] = va + hh
    return np.clip(val, 0, 2 * H - 1) if clamp else val


def stopped(keys, x, q, bpv, K, j):
    """the full-resolution inverse over sublevels 47 .. 3 j only -> (rows of the first leaves of the cells of lod j, in
    Morton order, not clamped)"""
    H = 1 << (8 * bpv - 1)
    x = np.asarray(x, np.int64)
    n = x.shape[0]
    q = _steps(q, x.shape[1], bpv)
    val = np.zeros_like(x)
    val[0] = x[0] + H
    b = sublevels(keys)
    g = kcells(keys, 0, K)
    M = scale(n, int(g[n]))
    for t in range(TOP - 1, 3 * j - 1, -1):
        at, lo, wa, wb = pairs(keys, b, t)
        if at.shape[0] == 0:
            continue
        if t >= 3 * K:
            ca, cb = g[at] - g[lo], g[at + wb] - g[at]
            hh = x[at] * _step_w(q, ca, cb, M)
            va = val[lo] - (cb[:, None] * hh) // (ca + cb)[:, None]
        else:
            hh = x[at] * _step_l(q, t)
            va = val[lo] - (hh >> 1)
        val[lo] = va
        val[at] = va + hh
    return val[b >= 3 * j]


def counts_of(keys):
    s = np.minimum(sublevels(keys) // 3, 16)
    return [int((s >= k).sum()) for k in range(16)]


def encode(points, values, bpv, q, K, colour=0, bias=32768):
    v = _as2d(values)
    n, c = v.shape
    q = _steps(q, c, bpv)
    _check_colour(colour, c)
    slod = _slod(bias)
    _check_k(K, slod)
    assert n == 0 or (v.min() >= 0 and v.max() < 1 << (8 * bpv))
    head = bytes([ord("A"), VERSION, bpv | (slod << 4), c]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    keys, v = _sorted(points, v, bias)
    if colour:
        v = colour_forward(v, bpv)
    x = forward(keys, v, q, bpv, K)
    body = struct.pack("<I", colour) + struct.pack("<%dI" % c, *q.tolist()) + struct.pack("<I", K)
    body += struct.pack("<16I", *counts_of(keys)) + _code(x[order_of(sublevels(keys))], bpv)
    return head + struct.pack("<I", len(body)) + body


def info(blob):
    assert len(blob) >= HEAD and blob[0] == ord("A") and blob[1] == VERSION, "not an attribute blob of version 22"
    bpv, c, n = blob[2] & 15, blob[3], struct.unpack_from("<I", blob, 4)[0]
    assert bpv in (1, 2) and 1 <= c <= 4
    q, colour, K = (0,) * c, 0, 0
    if n:
        assert len(blob) >= HEAD + 8 + 4 * c, "truncated in front of scalable_to"
        colour = struct.unpack_from("<I", blob, HEAD)[0]
        q = struct.unpack_from("<%dI" % c, blob, HEAD + 4)
        K = struct.unpack_from("<I", blob, HEAD + 4 + 4 * c)[0]
        _steps(q, c, bpv)
        _check_colour(colour, c)
        _check_k(K, blob[2] >> 4)
    return {"version": VERSION, "bpv": bpv, "channels": c, "points": n, "qstep": tuple(int(s) for s in q),
            "colour": "ycocg" if colour else None, "max_error": 0, "scalable": True, "scalable_to": K, "lod": blob[2] >> 4}


def _as_v2(blob):
    """(version 2's head over the blob's counts, S, chunks — what attr2_ref reads; the bytes this kind has in front)"""
    i = info(blob)
    x = 8 + 4 * i["channels"]                                              # the colour word, the steps and K
    plen = struct.unpack_from("<I", blob, 8)[0]
    return bytes([blob[0], 2, i["bpv"], i["channels"]]) + blob[4:8] + struct.pack("<I", plen - x) + blob[HEAD + x:], x


def lod_info(blob, lod):
    """(bytes, values): blob[:bytes] is the shortest prefix that decodes at `lod` (0 .. scalable_to)"""
    i = info(blob)
    if i["points"] == 0:
        return HEAD, 0
    assert 0 <= lod <= i["scalable_to"], "lod %d beyond scalable_to %d" % (lod, i["scalable_to"])
    b2, x = _as_v2(blob)
    nbytes, m = attr2_ref.lod_info(b2, lod)
    return nbytes + x, m


def indices(blob, m):
    """the first m coded indices [m, c] in coding order"""
    b2, _ = _as_v2(blob)
    return attr2_ref._residuals(b2, m)[0]


def decode(blob, cells, lod=0):
    i = info(blob)
    bpv, c, n, K = i["bpv"], i["channels"], i["points"], i["scalable_to"]
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    m = cells.shape[0]
    if n == 0:
        assert struct.unpack_from("<I", blob, 8)[0] == 0 and m == 0
        return np.zeros((0, c), np.int64), bpv
    assert 0 <= lod <= K, "lod %d beyond scalable_to %d" % (lod, K)
    counts = struct.unpack_from("<16I", blob, HEAD + 8 + 4 * c)
    assert m == counts[lod], "the blob has %d values at lod %d, the geometry %d cells" % (counts[lod], lod, m)
    assert len(blob) >= lod_info(blob, lod)[0], "truncated"
    kappa = np.sort(attr2_ref.keys_of(cells, 32768 >> (i["lod"] + lod)))
    x = np.zeros((m, c), np.int64)
    x[order_of(sublevels(kappa))] = indices(blob, m)
    out = inverse(kappa, x, i["qstep"], bpv, K, lod, n, counts[K])
    return (colour_inverse(out, bpv) if i["colour"] else out), bpv


def reconstruct(points, values, bpv, q, K, colour=0, bias=32768, lod=0):
    """what decode returns at `lod` for encode's blob, without the entropy stage"""
    keys, v = _sorted(points, values, bias)
    if v.shape[0] == 0:
        return v
    if colour:
        v = colour_forward(v, bpv)
    x = forward(keys, v, q, bpv, K)
    b = sublevels(keys)
    kappa = keys[b >= 3 * lod] >> np.uint64(3 * lod)
    g = kcells(keys, 0, K)
    out = inverse(kappa, x[b >= 3 * lod], q, bpv, K, lod, keys.shape[0], int(g[-1]))
    return colour_inverse(out, bpv) if colour else out
