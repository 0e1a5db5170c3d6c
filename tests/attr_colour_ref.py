"""A second statement of the transform-coded attribute blob with a colour transform and one step per channel, version
21 (the rule in include/pcc.h, the layout in csrc/attr_blob.h's header), written from that description in numpy.  It
takes from tests/attr_transform_ref.py what the two kinds share by definition (sublevels, pairs, the coding order, the
integer root, and the entropy stage _code) and has its own lifting passes with a step per channel, and the colour
transform.  Not a port of the kernels.

    colour_forward(v, bpv)                                      -> [n, c]: Y, Co, Cg in channels 0, 1, 2, the rest as it was
    colour_inverse(v, bpv)                                      -> R, G, B back, clamped to the value width
    forward(keys, v, q, bpv)                                    -> x int64 [n, c] by Morton index; q one step per channel
    inverse(keys, x, q, bpv)                                    -> values int64 [n, c], clamped to the value width
    encode(points, values, bpv, q, colour=0, bias=32768)        -> blob; q an integer (every channel) or c integers
    decode(blob, cells)                                         -> (values int64 [n, c], bpv)
    reconstruct(points, values, bpv, q, colour=0, bias=32768)   -> what decode returns for encode's blob
    info(blob)                                                  -> dict(version, bpv, channels, points, qstep (a tuple),
                                                                   colour ("ycocg" | None), max_error, scalable, lod)
    indices(blob)                                               -> the coded indices [n, c] in coding order
"""
import struct

import numpy as np

import attr2_ref
from attr_ref import HEAD, _as2d, layout
from attr_transform_ref import TOP, _code, _isqrt, _slod, _sorted, order_of, pairs, sublevels

VERSION = 21


def colour_forward(v, bpv):
    H = 1 << (8 * bpv - 1)
    out = np.array(v, np.int64)
    assert out.ndim == 2 and out.shape[1] >= 3
    r, g, b = out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    out[:, 0] = t + (cg >> 1)
    out[:, 1] = (co >> 1) + H
    out[:, 2] = (cg >> 1) + H
    assert out.shape[0] == 0 or (out[:, :3].min() >= 0 and out[:, :3].max() <= 2 * H - 1)
    return out


def colour_inverse(v, bpv):
    H = 1 << (8 * bpv - 1)
    out = np.clip(np.array(v, np.int64), 0, 2 * H - 1)
    co = 2 * (out[:, 1] - H)
    cg = 2 * (out[:, 2] - H)
    t = out[:, 0] - (cg >> 1)
    g = cg + t
    b = t - (co >> 1)
    out[:, 0], out[:, 1], out[:, 2] = b + co, g, b
    return np.clip(out, 0, 2 * H - 1)


def _steps(q, c, bpv):
    q = [q] * c if isinstance(q, (int, np.integer)) else list(q)
    assert len(q) == c, "%d steps for %d channels" % (len(q), c)
    for s in q:
        assert isinstance(s, (int, np.integer)) and 1 <= s < 1 << (8 * bpv - 1), "qstep %r with %d bytes per value" % (s, bpv)
    return np.array([int(s) for s in q], np.int64)


def step(q, wa, wb):
    """[pairs, c]: s[ch] = max(2, isqrt(floor(q[ch]^2 w / (wa wb))))"""
    wa, wb = np.asarray(wa, np.int64)[:, None], np.asarray(wb, np.int64)[:, None]
    v = (q * q)[None, :] * (wa + wb) // (wa * wb)
    return np.maximum(2, _isqrt(v.reshape(-1)).reshape(v.shape))


def forward(keys, v, q, bpv):
    H = 1 << (8 * bpv - 1)
    val = np.array(v, np.int64)
    q = _steps(q, val.shape[1], bpv)
    x = np.zeros_like(val)
    b = sublevels(keys)
    for t in range(TOP):
        at, lo, wa, wb = pairs(keys, b, t)
        if at.shape[0] == 0:
            continue
        h = val[at] - val[lo]
        val[lo] += (wb[:, None] * h) // (wa + wb)[:, None]
        s = step(q, wa, wb)
        x[at] = np.sign(h) * np.minimum((np.abs(h) + s // 2) // s, H - 1)
    x[0] = val[0] - H
    return x


def inverse(keys, x, q, bpv):
    H = 1 << (8 * bpv - 1)
    x = np.asarray(x, np.int64)
    q = _steps(q, x.shape[1], bpv)
    val = np.zeros_like(x)
    val[0] = x[0] + H
    b = sublevels(keys)
    for t in range(TOP - 1, -1, -1):
        at, lo, wa, wb = pairs(keys, b, t)
        if at.shape[0] == 0:
            continue
        hh = x[at] * step(q, wa, wb)
        va = val[lo] - (wb[:, None] * hh) // (wa + wb)[:, None]
        val[lo] = va
        val[at] = va + hh
    return np.clip(val, 0, 2 * H - 1)


def _check_colour(colour, c):
    assert colour in (0, 1), "colour %r" % (colour,)
    assert not colour or c >= 3, "the colour transform needs 3 channels, the frame has %d" % c


def encode(points, values, bpv, q, colour=0, bias=32768):
    v = _as2d(values)
    n, c = v.shape
    q = _steps(q, c, bpv)
    _check_colour(colour, c)
    assert n == 0 or (v.min() >= 0 and v.max() < 1 << (8 * bpv))
    head = bytes([ord("A"), VERSION, bpv | (_slod(bias) << 4), c]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    keys, v = _sorted(points, v, bias)
    if colour:
        v = colour_forward(v, bpv)
    x = forward(keys, v, q, bpv)
    body = struct.pack("<I", colour) + struct.pack("<%dI" % c, *q.tolist()) + _code(x[order_of(sublevels(keys))], bpv)
    return head + struct.pack("<I", len(body)) + body


def reconstruct(points, values, bpv, q, colour=0, bias=32768):
    keys, v = _sorted(points, values, bias)
    if v.shape[0] == 0:
        return v
    _check_colour(colour, v.shape[1])
    if colour:
        v = colour_forward(v, bpv)
    out = inverse(keys, forward(keys, v, q, bpv), q, bpv)
    return colour_inverse(out, bpv) if colour else out


def info(blob):
    assert len(blob) >= HEAD and blob[0] == ord("A") and blob[1] == VERSION, "not an attribute blob of version 21"
    bpv, c, n = blob[2] & 15, blob[3], struct.unpack_from("<I", blob, 4)[0]
    q, colour = (0,) * c, 0
    if n:
        colour = struct.unpack_from("<I", blob, HEAD)[0]
        q = struct.unpack_from("<%dI" % c, blob, HEAD + 4)
        _steps(q, c, bpv)
        _check_colour(colour, c)
    return {"version": VERSION, "bpv": bpv, "channels": c, "points": n, "qstep": tuple(int(s) for s in q),
            "colour": "ycocg" if colour else None, "max_error": 0, "scalable": False, "lod": blob[2] >> 4}


def indices(blob):
    """the coded indices [n, c] in coding order, through attr2_ref's reader: the same lanes, contexts and words under
    version 2's head, whose 16 counts this layout does not have"""
    i = info(blob)
    bpv, c, n = i["bpv"], i["channels"], i["points"]
    plen = struct.unpack_from("<I", blob, 8)[0]
    assert HEAD + plen == len(blob)
    x = 4 + 4 * c                                                          # the colour word and the steps
    counts = [n]
    for _ in range(15):
        counts.append(max(1, -(-counts[-1] // 8)))
    b2 = bytes([blob[0], 2, bpv, c]) + blob[4:8] + struct.pack("<I", plen - x + 64) + struct.pack("<16I", *counts) + blob[HEAD + x:]
    assert struct.unpack_from("<II", blob, HEAD + x) == layout(n, c)
    return attr2_ref._residuals(b2, n)[0]


def decode(blob, cells):
    i = info(blob)
    bpv, c, n = i["bpv"], i["channels"], i["points"]
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    assert cells.shape[0] == n, "the blob has %d values, the geometry %d points" % (n, cells.shape[0])
    if n == 0:
        assert struct.unpack_from("<I", blob, 8)[0] == 0
        return np.zeros((0, c), np.int64), bpv
    keys = np.sort(attr2_ref.keys_of(cells, 32768 >> i["lod"]))
    x = np.zeros((n, c), np.int64)
    x[order_of(sublevels(keys))] = indices(blob)
    out = inverse(keys, x, i["qstep"], bpv)
    return (colour_inverse(out, bpv) if i["colour"] else out), bpv
