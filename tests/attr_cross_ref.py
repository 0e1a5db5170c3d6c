"""A second statement of the cross-channel attribute blobs, versions 8, 11, 13 and 14 (the rule in include/pcc.h and in
csrc/attr_blob.h's header), written from that description in numpy on top of tests/attr_ref.py, attr2_ref.py and
attr_nl_ref.py: what the plain kind would code, w, comes from those refs (version 1's run residuals, version 2's
residuals in introduction order, the indices of versions 4 and 7), a channel of the mask is replaced by its wrapped
difference to the ORIGINAL w of the channel before it, and the result goes through attr_nl_ref's coder, which codes what
it is handed with the bucket of the channel's previous magnitude as context.  The decoder reads the differences with
attr2_ref's reader, undoes them channel by channel in ascending order, and finishes as the plain kind does.  Not a
port of the kernels.

    mask_of(cross, c)                                       -> m: cross True (every channel 1 .. c - 1), a sequence of
                                                               channel indices, or m itself
    forward(w, m, bpv) / inverse(x, m, bpv)                 -> x / w, int64 [n, c] in [-h, h)
    encode(values, bpv, cross, e=0, points=None, bias=32768) -> blob: version 8 / 13 (points None, e = 0 / e > 0; values
                                                               in Morton order) or 11 / 14 (points int [n, 3] distinct,
                                                               any order); an empty mask: the plain kind's blob
    decode(blob_or_prefix, cells=None, lod=0)               -> (values int64 [m, c], bpv); plain kinds pass through
    lod_info(blob_or_prefix, lod)                           -> (bytes, values) of a version 11 / 14 (or 2 / 7) blob
    info(blob)                                              -> attr_nl_ref.info's dict, for a cross kind with its own
                                                               version and cross_channel, a tuple of channel indices
encode takes layout=(S, n_chunks) and p0=, decode and lod_info any_layout=True, as attr_nl_ref's do.
"""
import struct

import numpy as np

import attr2_ref
import attr_nl_ref
import attr_ref
from attr_ref import HEAD, LANES, _as2d, pick_layout

CROSS_OF = {1: 8, 2: 11, 4: 13, 7: 14}
PLAIN_OF = {v: k for k, v in CROSS_OF.items()}


def mask_of(cross, c):
    if cross is True:
        return (1 << (c - 1)) - 1
    if cross is False or cross is None:
        return 0
    if isinstance(cross, (int, np.integer)):
        m = int(cross)
    else:
        chans = [int(ch) for ch in cross]
        assert len(set(chans)) == len(chans) and all(1 <= ch <= 3 for ch in chans)
        m = sum(1 << (ch - 1) for ch in chans)
    assert 0 <= m < 1 << (c - 1), "mask %d with %d channels" % (m, c)
    return m


def _wrap(d, bpv):
    half, mask = 1 << (8 * bpv - 1), (1 << (8 * bpv)) - 1
    return ((d + half) & mask) - half


def forward(w, m, bpv):
    x = w.copy()
    for ch in range(1, w.shape[1]):
        if m >> (ch - 1) & 1:
            x[:, ch] = _wrap(w[:, ch] - w[:, ch - 1], bpv)                  # against w, not against x
    return x


def inverse(x, m, bpv):
    w = x.copy()
    for ch in range(1, x.shape[1]):                                         # ascending: w[ch - 1] is complete
        if m >> (ch - 1) & 1:
            w[:, ch] = _wrap(x[:, ch] + w[:, ch - 1], bpv)
    return w


def _runs(a, n, c, given=None):
    S, nc = pick_layout(n, c, given)
    runs = np.zeros((nc * LANES * S, c), np.int64)
    runs[:n] = a
    return runs.reshape(nc * LANES, S, c)


def encode(values, bpv, cross, e=0, points=None, bias=32768, layout=None, p0=None):
    v = _as2d(values)
    n, c = v.shape
    m = mask_of(cross, c)
    if m == 0:
        return attr_nl_ref.encode(v, bpv, e, points, bias, layout, p0)
    scal, nl = points is not None, e > 0
    if nl:
        attr_nl_ref._check_e(e, bpv)
    assert n == 0 or (v.min() >= 0 and v.max() < 1 << (8 * bpv))
    slod = 15 - int(bias).bit_length() + 1 if scal else 0
    assert bias == 32768 >> slod
    ver = CROSS_OF[(7 if nl else 2) if scal else (4 if nl else 1)]
    head = bytes([ord("A"), ver, bpv | (slod << 4), c | (m << 4)]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    body = struct.pack("<I", e) if nl else b""
    if not scal:                                                            # the lane runs of the Morton order
        w = attr_nl_ref.indices4(v, e, layout)[0] if nl else attr_ref._resid(_runs(v, n, c, layout), bpv)[0].reshape(-1, c)[:n]
    else:                                                                   # the introduction order
        keys = attr2_ref.keys_of(points, bias)
        srt = np.argsort(keys, kind="stable")
        keys, v = keys[srt], v[srt]
        s, order, first = attr2_ref.intro(keys)
        if nl:
            w = attr_nl_ref.indices7(v, s, first, e)[0][order]
        else:
            pred = v[first]
            pred[0] = 0
            w = _wrap(v - pred, bpv)[order]
        body += struct.pack("<16I", *[int((s >= k).sum()) for k in range(16)])
    body += attr_nl_ref._code(forward(w, m, bpv), bpv, layout, p0)
    return head + struct.pack("<I", len(body)) + body


def _plain_head(blob):
    """a cross blob (or prefix) under the head of its plain kind: the same layout, the mask taken out of byte 3"""
    assert len(blob) >= HEAD and blob[0] == ord("A") and blob[1] in PLAIN_OF, "not a cross-channel attribute blob"
    c, m = blob[3] & 15, blob[3] >> 4
    assert 2 <= c <= 4 and 0 < m < 1 << (c - 1), "mask %d with %d channels" % (m, c)
    return bytes([blob[0], PLAIN_OF[blob[1]], blob[2], c]) + blob[4:], m


def info(blob):
    if blob[1] not in PLAIN_OF:
        assert len(blob) < 4 or blob[1] not in CROSS_OF or blob[3] >> 4 == 0
        return attr_nl_ref.info(blob)
    plain, m = _plain_head(blob)
    i = attr_nl_ref.info(plain)
    i["version"] = blob[1]
    i["cross_channel"] = tuple(ch for ch in range(1, 4) if m >> (ch - 1) & 1)
    return i


def lod_info(blob, lod, any_layout=False):
    if blob[1] not in PLAIN_OF:
        return attr_nl_ref.lod_info(blob, lod, any_layout)
    assert blob[1] in (11, 14)
    return attr_nl_ref.lod_info(_plain_head(blob)[0], lod, any_layout)


def decode(blob, cells=None, lod=0, any_layout=False):
    if blob[1] not in PLAIN_OF:
        return attr_nl_ref.decode(blob, cells, lod, any_layout)
    i = info(blob)
    m = _plain_head(blob)[1]
    bpv, c, n, e = i["bpv"], i["channels"], i["points"], i["max_error"]
    scal, nl = i["scalable"], blob[1] in (13, 14)
    mask, q = (1 << (8 * bpv)) - 1, 2 * e + 1
    plen = struct.unpack_from("<I", blob, 8)[0]
    if n == 0:
        assert plen == 0 and len(blob) == HEAD and (cells is None or np.asarray(cells).size == 0)
        return np.zeros((0, c), np.int64), bpv
    # the differences through attr2_ref's reader: the same lanes, contexts and words under version 2's head, max_error
    # taken out and, for the unscalable kinds, 16 counts put in that their layout does not have
    body, x4 = (blob[HEAD + 4:], 4) if nl else (blob[HEAD:], 0)
    if not scal:
        assert cells is None and lod == 0 and HEAD + plen == len(blob)
        counts = [n]
        for _ in range(15):
            counts.append(max(1, -(-counts[-1] // 8)))
        b2 = bytes([blob[0], 2, bpv, c]) + blob[4:8] + struct.pack("<I", plen - x4 + 64) + struct.pack("<16I", *counts) + body
        x = attr2_ref._residuals(b2, n, any_layout)[0]
        w = _runs(inverse(x, m, bpv), n, c, struct.unpack_from("<II", blob, HEAD + x4))   # the header's: checked by the reader
        vh = np.zeros_like(w)
        for s in range(w.shape[1]):                                         # all runs side by side
            p = 0 if s == 0 else (vh[:, 0] if s == 1 else (vh[:, s - 1] + vh[:, s - 2] + 1) >> 1)
            vh[:, s] = p + w[:, s] * q if nl else (p + w[:, s]) & mask
        vh = vh.reshape(-1, c)[:n]
    else:
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        b2 = bytes([blob[0], 2, blob[2], c]) + blob[4:8] + struct.pack("<I", plen - x4) + body
        _, _, _, h = attr2_ref._header(b2, any_layout)
        k = cells.shape[0]
        assert k == h[0][lod], "the blob has %d values at lod %d, the geometry %d cells" % (h[0][lod], lod, k)
        assert len(b2) >= attr2_ref.lod_info(b2, lod, any_layout)[0], "truncated"
        x = attr2_ref._residuals(b2, k, any_layout)[0]
        assert h[5] + lod <= 15
        keys = np.sort(attr2_ref.keys_of(cells, 32768 >> (h[5] + lod)))
        s, order, first = attr2_ref.intro(keys)
        assert [int((s >= j).sum()) for j in range(16 - lod)] == list(h[0][lod:]), "the cells do not give the header's counts"
        w = np.zeros((k, c), np.int64)
        w[order] = inverse(x, m, bpv)                                       # w of every Morton index
        tot = np.zeros((k, c), np.int64)
        tot[0] = w[0]
        for size in range(15, -1, -1):                                      # sums along the chains, coarsest first
            at = np.nonzero((s == size) & (np.arange(k) > 0))[0]
            tot[at] = tot[first[at]] + w[at]
        vh = tot * q if nl else tot & mask
    if nl:
        assert (vh >= -e).all() and (vh <= mask + e).all(), "a reconstruction no encoder produces"
        vh = np.clip(vh, 0, mask)
    return vh, bpv
