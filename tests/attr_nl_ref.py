"""A second statement of the near-lossless attribute blobs, versions 4 and 7 (the rule in include/pcc.h, the layout in
csrc/attr_blob.h's header), written from that description in numpy on top of tests/attr_ref.py and tests/attr2_ref.py:
the closed loop of version 4 stepped over all lane runs side by side (one numpy step per run position), the chains of
version 7 resolved size by size (coarsest first) instead of walked per point, the entropy stage as attr_ref states it
(its slots, p0 and adaptation imported).  What the lanes code is the index j of the quantised prediction error; a
near-lossless blob is the lossless layout of its kind over those indices with max_error behind payload_len, so the
decoder here strips that word and reads the indices with attr2_ref's reader.  Not a port of the kernels.

    quantise(d, e)                                   -> j = sgn(d) floor((|d| + e) / (2 e + 1))
    encode(values, bpv, e, points=None, bias=32768)  -> blob: version 4 (points None: values [n] / [n, c] in Morton order)
                                                        or version 7 (points int [n, 3] distinct, any order, row i of
                                                        values belonging to points[i]); e = 0: the lossless blob of
                                                        attr_ref / attr2_ref
    decode(blob_or_prefix, cells=None, lod=0)        -> (values int64 [m, c], bpv): version 4 (cells None) or version 7
                                                        (cells as attr2_ref.decode takes them); lossless blobs pass
                                                        through to attr_ref / attr2_ref
    lod_info(blob_or_prefix, lod)                    -> (bytes, values) of a version 7 (or 2) blob
    info(blob)                                       -> dict(version, bpv, channels, points, max_error, scalable, lod)
encode takes layout=(S, n_chunks) and p0= as attr_ref.encode does (version 4's closed loop runs over the lanes of that
layout); decode and lod_info take any_layout=True as attr2_ref's do, without it they insist on the encoder's layout.
"""
import struct

import numpy as np

import attr2_ref
import attr_ref
from attr_ref import HEAD, L, LANES, _adapt, _as2d, _bucket, _p0, _slots, contexts, pick_layout, pick_p0


def quantise(d, e):
    d = np.asarray(d, np.int64)
    return np.sign(d) * ((np.abs(d) + e) // (2 * e + 1))


def _check_e(e, bpv):
    assert isinstance(e, (int, np.integer)) and 1 <= e < 1 << (8 * bpv - 1), "max_error %r with %d bytes per value" % (e, bpv)


def _code(r, bpv, layout=None, p0=None):
    """indices r int64 [n, c] in coding order, n > 0 -> S | n_chunks | p0 | chunk table | chunk payloads: r dealt to lanes
    and chunks, each lane coding its run with the bucket of the channel's previous |r| in the run as context"""
    n, c = r.shape
    S, nc = pick_layout(n, c, layout)
    R = nc * LANES
    runs = np.zeros((R * S, c), np.int64)
    runs[:n] = r
    runs = runs.reshape(R, S, c)
    valid = (np.arange(R * S) < n).reshape(R, S)
    bk = np.zeros_like(runs)
    bk[:, 1:] = _bucket(np.abs(runs[:, :-1]))
    nctx = contexts(bpv, c)
    c0 = np.zeros(nctx, np.int64)
    c1 = np.zeros(nctx, np.int64)
    per = []
    for k in range(0, R, LANES):                                            # a chunk's 64 runs at a time (memory)
        ctx, bit, ok = _slots(runs[k:k + LANES], bk[k:k + LANES], valid[k:k + LANES], bpv)
        c1 += np.bincount(ctx[ok & (bit == 1)], minlength=nctx)
        c0 += np.bincount(ctx[ok & (bit == 0)], minlength=nctx)
        Kc = ok.sum(1)
        o = np.argsort(~ok, axis=1, kind="stable")[:, :Kc.max()]            # every run's coded decisions first
        per.append((np.take_along_axis(ctx, o, 1), np.take_along_axis(bit, o, 1), Kc))
    p0 = pick_p0(_p0(c0, c1), p0)
    K = np.concatenate([p[2] for p in per])
    T = int(K.max())
    cx = np.zeros((R, T), np.int64)
    bt = np.zeros((R, T), np.int64)
    for k, (a, b, _) in enumerate(per):
        cx[k * LANES:(k + 1) * LANES, :a.shape[1]] = a
        bt[k * LANES:(k + 1) * LANES, :b.shape[1]] = b
    lanes = np.arange(R)
    model = np.tile(p0, (R, 1))
    prob = np.zeros_like(cx)
    for t in range(T):                                                      # forward: the models, every lane from p0
        act = t < K
        p = model[lanes, cx[:, t]]
        prob[:, t] = p
        model[lanes[act], cx[act, t]] = _adapt(p, bt[:, t])[act]
    x = np.full(R, L, np.int64)
    words = np.zeros((R, T), np.int64)
    cnt = np.zeros(R, np.int64)
    for t in range(T - 1, -1, -1):                                          # backward: rANS, 16-bit words
        act = t < K
        p1, b = prob[:, t], bt[:, t]
        freq = np.where(b == 1, p1, 4096 - p1)
        start = np.where(b == 1, 4096 - p1, 0)
        need = act & (x >= (freq << 20))
        words[lanes[need], cnt[need]] = x[need] & 0xFFFF
        cnt += need
        x = np.where(need, x >> 16, x)
        x = np.where(act, ((x // freq) << 12) + x % freq + start, x)
    chunks = []
    for k in range(nc):
        ls = range(k * LANES, (k + 1) * LANES)
        st = [w for l in ls for w in (int(x[l]) & 0xFFFF, int(x[l]) >> 16)]
        run = [int(w) for l in ls for w in words[l, :cnt[l]][::-1]]         # the order the decoder takes them
        chunks.append(st + [int(cnt[l]) for l in ls] + run)
    body = struct.pack("<II", S, nc) + struct.pack("<%dH" % nctx, *p0.tolist())
    body += b"".join(struct.pack("<I", len(ch)) for ch in chunks)
    return body + b"".join(struct.pack("<%dH" % len(ch), *ch) for ch in chunks)


def indices4(v, e, layout=None):
    """version 4: merged values v int64 [n, c] in Morton order -> (j [n, c], v^ [n, c] unclamped)"""
    n, c = v.shape
    S, nc = pick_layout(n, c, layout)
    R = nc * LANES
    runs = np.zeros((R * S, c), np.int64)
    runs[:n] = v
    runs = runs.reshape(R, S, c)
    q = 2 * e + 1
    j = np.zeros_like(runs)
    vh = np.zeros_like(runs)
    for s in range(S):                                                      # all runs side by side
        p = 0 if s == 0 else (vh[:, 0] if s == 1 else (vh[:, s - 1] + vh[:, s - 2] + 1) >> 1)
        j[:, s] = quantise(runs[:, s] - p, e)
        vh[:, s] = p + j[:, s] * q
    return j.reshape(-1, c)[:n], vh.reshape(-1, c)[:n]


def indices7(v, s, first, e):
    """version 7: merged values v [n, c] in Morton order with their sizes of introduction and predictors (attr2_ref.intro)
    -> (j [n, c], v^ [n, c] unclamped), both by Morton index"""
    q = 2 * e + 1
    j = np.zeros_like(v)
    vh = np.zeros_like(v)
    j[0] = quantise(v[0], e)
    vh[0] = j[0] * q
    for size in range(15, -1, -1):                                          # a size's predictors are all coarser: done
        at = np.nonzero((s == size) & (np.arange(v.shape[0]) > 0))[0]
        j[at] = quantise(v[at] - vh[first[at]], e)
        vh[at] = vh[first[at]] + j[at] * q
    return j, vh


def encode(values, bpv, e, points=None, bias=32768, layout=None, p0=None):
    v = _as2d(values)
    n, c = v.shape
    if e == 0:
        return attr_ref.encode(v, bpv, layout, p0) if points is None else attr2_ref.encode(points, v, bpv, bias, layout, p0)
    _check_e(e, bpv)
    assert n == 0 or (v.min() >= 0 and v.max() < 1 << (8 * bpv))
    if points is None:
        head = bytes([ord("A"), 4, bpv, c]) + struct.pack("<I", n)
        if n == 0:
            return head + struct.pack("<I", 0)
        body = struct.pack("<I", e) + _code(indices4(v, e, layout)[0], bpv, layout, p0)
        return head + struct.pack("<I", len(body)) + body
    slod = 15 - int(bias).bit_length() + 1
    assert bias == 32768 >> slod
    head = bytes([ord("A"), 7, bpv | (slod << 4), c]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    keys = attr2_ref.keys_of(points, bias)
    srt = np.argsort(keys, kind="stable")
    keys, v = keys[srt], v[srt]
    s, order, first = attr2_ref.intro(keys)
    j, _ = indices7(v, s, first, e)
    cells = [int((s >= k).sum()) for k in range(16)]
    body = struct.pack("<I", e) + struct.pack("<16I", *cells) + _code(j[order], bpv, layout, p0)     # indices in introduction order
    return head + struct.pack("<I", len(body)) + body


def info(blob):
    assert len(blob) >= HEAD and blob[0] == ord("A") and blob[1] in (1, 2, 4, 7), "not an attribute blob"
    ver = blob[1]
    scal, nl = ver in (2, 7), ver in (4, 7)
    n = struct.unpack_from("<I", blob, 4)[0]
    e = 0
    if nl and n:
        e = struct.unpack_from("<I", blob, HEAD)[0]
        _check_e(e, blob[2] & 15 if scal else blob[2])
    return {"version": ver, "bpv": blob[2] & 15 if scal else blob[2], "channels": blob[3], "points": n, "max_error": e,
            "scalable": scal, "lod": blob[2] >> 4 if scal else 0}


def _lossless_shape(blob):
    """a version-7 blob or prefix -> (the version-2 blob or prefix over its indices, e): max_error taken out"""
    i = info(blob)
    assert i["version"] == 7
    n, plen = struct.unpack_from("<II", blob, 4)
    if n == 0:
        assert plen == 0
        return bytes([blob[0], 2]) + blob[2:HEAD], 0
    assert len(blob) >= HEAD + 4 and plen >= 4
    return bytes([blob[0], 2]) + blob[2:8] + struct.pack("<I", plen - 4) + blob[HEAD + 4:], i["max_error"]


def lod_info(blob, lod, any_layout=False):
    if blob[1] == 2:
        return attr2_ref.lod_info(blob, lod, any_layout)
    b2, _ = _lossless_shape(blob)
    nbytes, m = attr2_ref.lod_info(b2, lod, any_layout)
    return (nbytes + 4 if m else nbytes), m


def decode(blob, cells=None, lod=0, any_layout=False):
    ver = blob[1]
    if ver == 1:
        return attr_ref.decode(blob)
    if ver == 2:
        return attr2_ref.decode(blob, cells, lod, any_layout)
    i = info(blob)
    bpv, c, n, e = i["bpv"], i["channels"], i["points"], i["max_error"]
    mask, q = (1 << (8 * bpv)) - 1, 2 * e + 1
    if ver == 4:
        assert cells is None and lod == 0
        plen = struct.unpack_from("<I", blob, 8)[0]
        assert HEAD + plen == len(blob)
        if n == 0:
            assert plen == 0
            return np.zeros((0, c), np.int64), bpv
        # the indices through attr2_ref's reader: the same lanes, contexts and words under version 2's head, whose 16
        # counts (cells[0] = n, each at least an eighth of the one before) this layout does not have
        counts = [n]
        for _ in range(15):
            counts.append(max(1, -(-counts[-1] // 8)))
        b2 = bytes([blob[0], 2, bpv, c]) + blob[4:8] + struct.pack("<I", plen - 4 + 64) + struct.pack("<16I", *counts) + blob[HEAD + 4:]
        j = attr2_ref._residuals(b2, n, any_layout)[0]                      # signed, as the binarisation holds them
        S, nc = struct.unpack_from("<II", blob, HEAD + 4)                   # the header's: _residuals has checked them
        runs = np.zeros((nc * LANES * S, c), np.int64)
        runs[:n] = j
        runs = runs.reshape(nc * LANES, S, c)
        vh = np.zeros_like(runs)
        for s in range(S):
            p = 0 if s == 0 else (vh[:, 0] if s == 1 else (vh[:, s - 1] + vh[:, s - 2] + 1) >> 1)
            vh[:, s] = p + runs[:, s] * q
        vh = vh.reshape(-1, c)[:n]
        assert (vh >= -e).all() and (vh <= mask + e).all(), "a reconstruction no encoder produces"
        return np.clip(vh, 0, mask), bpv
    assert ver == 7
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    b2, e = _lossless_shape(blob)
    _, _, _, h = attr2_ref._header(b2, any_layout)
    m = cells.shape[0]
    if n == 0:
        assert m == 0
        return np.zeros((0, c), np.int64), bpv
    assert m == h[0][lod], "the blob has %d values at lod %d, the geometry %d cells" % (h[0][lod], lod, m)
    assert len(b2) >= attr2_ref.lod_info(b2, lod, any_layout)[0], "truncated"
    j = attr2_ref._residuals(b2, m, any_layout)[0]
    assert h[5] + lod <= 15
    keys = np.sort(attr2_ref.keys_of(cells, 32768 >> (h[5] + lod)))
    s, order, first = attr2_ref.intro(keys)
    assert [int((s >= k).sum()) for k in range(16 - lod)] == list(h[0][lod:]), "the cells do not give the header's counts"
    idx = np.zeros((m, c), np.int64)
    idx[order] = j                                                          # index of every Morton index
    tot = np.zeros((m, c), np.int64)
    tot[0] = idx[0]
    for size in range(15, -1, -1):                                          # sums of j along the chains, coarsest first
        at = np.nonzero((s == size) & (np.arange(m) > 0))[0]
        tot[at] = tot[first[at]] + idx[at]
    vh = tot * q
    assert (vh >= -e).all() and (vh <= mask + e).all(), "a reconstruction no encoder produces"
    return np.clip(vh, 0, mask), bpv
