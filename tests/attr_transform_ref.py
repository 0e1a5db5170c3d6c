"""A second statement of the transform-coded attribute blob, version 19 (the rule in include/pcc.h, the layout in
csrc/attr_blob.h's header), written from that description in numpy on top of tests/attr2_ref.py (keys) and
tests/attr_nl_ref.py (the entropy stage, _code): an integer lifting form of the region-adaptive hierarchical transform
over the binary splits of the Morton tree, one numpy step per sublevel with every pair of the sublevel side by side.
Not a port of the kernels.

    sublevels(keys)                                   -> b [n]: bit of the split that introduces point i (b[0] = 48)
    pairs(keys, t)                                    -> (at, lo, wa, wb) of the pairs of sublevel t
    step(q, wa, wb)                                   -> s = max(2, isqrt(floor(q^2 (wa + wb) / (wa wb))))
    forward(keys, v, q, bpv)                          -> x int64 [n, c] by Morton index (x[0]: the weighted mean - H)
    inverse(keys, x, q, bpv)                          -> values int64 [n, c], clamped to the value width
    encode(points, values, bpv, q, bias=32768)        -> blob; points int [n, 3] distinct (any order), row i of values
                                                         belonging to points[i]
    decode(blob, cells)                               -> (values int64 [n, c], bpv): cells int [n, 3] = the frame's
                                                         distinct points (any order); row j the j-th in Morton order
    reconstruct(points, values, bpv, q, bias=32768)   -> what decode returns for encode's blob, without the entropy stage
    info(blob)                                        -> dict(version, bpv, channels, points, qstep, max_error, scalable, lod)
"""
import struct

import numpy as np

import attr2_ref
from attr_nl_ref import _code
from attr_ref import HEAD, _as2d, layout

VERSION = 19
TOP = 48                       # b of a frame's first point: above every split


def sublevels(keys):
    k = np.asarray(keys).astype(np.int64)
    b = np.full(k.shape[0], TOP, np.int64)
    if k.shape[0] > 1:
        x = k[1:] ^ k[:-1]
        assert (k[1:] > k[:-1]).all(), "keys must be sorted and distinct"
        b[1:] = np.frexp(x.astype(np.float64))[1] - 1                      # float64 holds 48 bits exactly
    return b


def order_of(b):
    """Morton index of the j-th coded point: b descending, Morton index ascending (point 0 first)"""
    return np.argsort(-b, kind="stable")


def pairs(keys, b, t):
    k = np.asarray(keys).astype(np.int64)
    at = np.nonzero(b == t)[0]
    low = (1 << t) - 1
    lo = np.searchsorted(k, k[at] & ~((low << 1) | 1))
    hi = np.searchsorted(k, (k[at] | low) + 1)
    return at, lo, at - lo, hi - at


def _isqrt(v):
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r -= (r * r > v)
    r += ((r + 1) * (r + 1) <= v)
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return r


def step(q, wa, wb):
    wa, wb = np.asarray(wa, np.int64), np.asarray(wb, np.int64)
    return np.maximum(2, _isqrt(q * q * (wa + wb) // (wa * wb)))


def _check_q(q, bpv):
    assert isinstance(q, (int, np.integer)) and 1 <= q < 1 << (8 * bpv - 1), "qstep %r with %d bytes per value" % (q, bpv)


def forward(keys, v, q, bpv):
    H = 1 << (8 * bpv - 1)
    val = np.array(v, np.int64)
    x = np.zeros_like(val)
    b = sublevels(keys)
    for t in range(TOP):
        at, lo, wa, wb = pairs(keys, b, t)
        if at.shape[0] == 0:
            continue
        h = val[at] - val[lo]
        val[lo] += (wb[:, None] * h) // (wa + wb)[:, None]                 # floor towards -inf
        s = step(q, wa, wb)[:, None]
        x[at] = np.sign(h) * np.minimum((np.abs(h) + s // 2) // s, H - 1)
    x[0] = val[0] - H
    return x


def inverse(keys, x, q, bpv):
    H = 1 << (8 * bpv - 1)
    x = np.asarray(x, np.int64)
    val = np.zeros_like(x)
    val[0] = x[0] + H
    b = sublevels(keys)
    for t in range(TOP - 1, -1, -1):
        at, lo, wa, wb = pairs(keys, b, t)
        if at.shape[0] == 0:
            continue
        hh = x[at] * step(q, wa, wb)[:, None]
        va = val[lo] - (wb[:, None] * hh) // (wa + wb)[:, None]
        val[lo] = va
        val[at] = va + hh
    return np.clip(val, 0, 2 * H - 1)


def _sorted(points, values, bias):
    v = _as2d(values)
    keys = attr2_ref.keys_of(points, bias)
    srt = np.argsort(keys, kind="stable")
    return keys[srt], v[srt]


def _slod(bias):
    slod = 15 - int(bias).bit_length() + 1
    assert bias == 32768 >> slod
    return slod


def encode(points, values, bpv, q, bias=32768):
    v = _as2d(values)
    n, c = v.shape
    _check_q(q, bpv)
    assert n == 0 or (v.min() >= 0 and v.max() < 1 << (8 * bpv))
    head = bytes([ord("A"), VERSION, bpv | (_slod(bias) << 4), c]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    keys, v = _sorted(points, v, bias)
    x = forward(keys, v, q, bpv)
    body = struct.pack("<I", q) + _code(x[order_of(sublevels(keys))], bpv)
    return head + struct.pack("<I", len(body)) + body


def reconstruct(points, values, bpv, q, bias=32768):
    keys, v = _sorted(points, values, bias)
    if v.shape[0] == 0:
        return v
    return inverse(keys, forward(keys, v, q, bpv), q, bpv)


def info(blob):
    assert len(blob) >= HEAD and blob[0] == ord("A") and blob[1] == VERSION, "not an attribute blob of version 19"
    bpv, n = blob[2] & 15, struct.unpack_from("<I", blob, 4)[0]
    q = 0
    if n:
        q = struct.unpack_from("<I", blob, HEAD)[0]
        _check_q(q, bpv)
    return {"version": VERSION, "bpv": bpv, "channels": blob[3], "points": n, "qstep": q, "max_error": 0, "scalable": False,
            "lod": blob[2] >> 4}


def indices(blob):
    """the coded indices [n, c] in coding order, through attr2_ref's reader: the same lanes, contexts and words under
    version 2's head, whose 16 counts this layout does not have"""
    i = info(blob)
    bpv, c, n = i["bpv"], i["channels"], i["points"]
    plen = struct.unpack_from("<I", blob, 8)[0]
    assert HEAD + plen == len(blob)
    counts = [n]
    for _ in range(15):
        counts.append(max(1, -(-counts[-1] // 8)))
    b2 = bytes([blob[0], 2, bpv, c]) + blob[4:8] + struct.pack("<I", plen - 4 + 64) + struct.pack("<16I", *counts) + blob[HEAD + 4:]
    assert struct.unpack_from("<II", blob, HEAD + 4) == layout(n, c)
    return attr2_ref._residuals(b2, n)[0]


def decode(blob, cells):
    i = info(blob)
    bpv, c, n, q = i["bpv"], i["channels"], i["points"], i["qstep"]
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    assert cells.shape[0] == n, "the blob has %d values, the geometry %d points" % (n, cells.shape[0])
    if n == 0:
        assert struct.unpack_from("<I", blob, 8)[0] == 0
        return np.zeros((0, c), np.int64), bpv
    keys = np.sort(attr2_ref.keys_of(cells, 32768 >> i["lod"]))
    x = np.zeros((n, c), np.int64)
    x[order_of(sublevels(keys))] = indices(blob)
    return inverse(keys, x, q, bpv), bpv
