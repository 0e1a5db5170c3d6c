"""A second statement of attribute blob version 2 (the layout in csrc/attr_blob.h's header), written from that
description in numpy: the introduction order by one stable argsort, the predictor by one searchsorted, the chains
resolved size by size (coarsest first) instead of walked per point, and the entropy stage as tests/attr_ref.py states
version 1's (fixed slots with a validity mask, all lanes stepped side by side).  Not a port of the kernels.

    encode(points, values, bpv, bias=32768) -> blob     points int [n, 3] distinct (any order), values int [n] / [n, c]
                                                        row i belonging to points[i]; bias 32768 >> k: the points
                                                        are the cells of a sender's side lod k; layout=(S, n_chunks)
                                                        and p0= as attr_ref.encode takes them
    decode(blob_or_prefix, cells, lod)      -> (values int64 [m, c], bpv): cells int [m, 3] = the distinct points >> lod
                                               (any order); row j belongs to the j-th cell in Morton order
    lod_info(blob_or_prefix, lod)           -> (bytes, values)
    status(blob_or_prefix, m)               -> the lane decoder's status word for the first m values (attr_ref.status)
decode, lod_info and status take any_layout=True: (S, n_chunks) may be any the parser accepts (attr_ref.check_layout);
without it they insist on the encoder's layout(n, c).
    intro(keys)                             -> (s, order, first) of Morton-sorted distinct keys
    keys_of(points, bias)                   -> 48-bit Morton keys (x bits at 3i + 2, y at 3i + 1, z at 3i)
"""
import struct

import numpy as np

from attr_ref import (BUCKETS, HEAD, L, LANES, _adapt, _as2d, _bucket, _p0, _slots, check_layout, contexts, layout, pick_layout, pick_p0,
                      positions)

HEAD2 = HEAD + 64 + 8          # 'A' 2 bpv c | n | payload_len | cells[16] | S | n_chunks


def _spread3(v):
    x = v.astype(np.uint64) & np.uint64(0xFFFF)
    for sh, m in ((16, 0x0000FF0000FF), (8, 0x00F00F00F00F), (4, 0x0C30C30C30C3), (2, 0x249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(m)
    return x


def keys_of(points, bias=32768):
    p = np.asarray(points, np.int64).reshape(-1, 3) + bias
    assert p.size == 0 or (p.min() >= 0 and p.max() < 65536)
    return (_spread3(p[:, 0]) << np.uint64(2)) | (_spread3(p[:, 1]) << np.uint64(1)) | _spread3(p[:, 2])


def intro(keys):
    """keys: sorted, distinct -> s [n] (size of introduction), order [n] (Morton index of the j-th introduced point),
    first [n] (the predictor's Morton index; first[0] = 0, unused)"""
    n = keys.shape[0]
    s = np.full(n, 16, np.int64)
    if n > 1:
        x = keys[1:] ^ keys[:-1]
        assert (x > 0).all(), "keys must be sorted and distinct"
        s[1:] = (np.frexp(x.astype(np.float64))[1] - 1) // 3          # float64 holds 48 bits exactly
    order = np.argsort(-s, kind="stable")
    low = (np.uint64(1) << (np.uint64(3) * (np.minimum(s, 15) + 1).astype(np.uint64))) - np.uint64(1)
    first = np.searchsorted(keys, keys & ~low)
    if n:
        first[0] = 0
    return s, order, first


def _runs(r, n, c, given=None):
    S, nc = pick_layout(n, c, given)
    R = nc * LANES
    runs = np.zeros((R * S, c), np.int64)
    runs[:n] = r
    runs = runs.reshape(R, S, c)
    valid = (np.arange(R * S) < n).reshape(R, S)
    bk = np.zeros_like(runs)
    bk[:, 1:] = _bucket(np.abs(runs[:, :-1]))
    return S, nc, runs, bk, valid


def encode(points, values, bpv, bias=32768, layout=None, p0=None):
    v = _as2d(values)
    n, c = v.shape
    slod = 15 - int(bias).bit_length() + 1
    assert bias == 32768 >> slod
    head = bytes([ord("A"), 2, bpv | (slod << 4), c]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    keys = keys_of(points, bias)
    srt = np.argsort(keys, kind="stable")
    keys, v = keys[srt], v[srt]
    s, order, first = intro(keys)
    half, mask = 1 << (8 * bpv - 1), (1 << (8 * bpv)) - 1
    pred = v[first]
    pred[0] = 0
    r = (((v - pred + half) & mask) - half)[order]                     # residuals in introduction order
    cells = [int((s >= k).sum()) for k in range(16)]
    S, nc, runs, bk, valid = _runs(r, n, c, layout)
    R = nc * LANES
    nctx = contexts(bpv, c)
    c0 = np.zeros(nctx, np.int64)
    c1 = np.zeros(nctx, np.int64)
    per = []
    for k in range(nc):
        sl = slice(k * LANES, (k + 1) * LANES)
        ctx, bit, ok = _slots(runs[sl], bk[sl], valid[sl], bpv)
        c1 += np.bincount(ctx[ok & (bit == 1)], minlength=nctx)
        c0 += np.bincount(ctx[ok & (bit == 0)], minlength=nctx)
        o = np.argsort(~ok, axis=1, kind="stable")
        K = ok.sum(1)
        per.append((np.take_along_axis(ctx, o, 1)[:, :K.max()], np.take_along_axis(bit, o, 1)[:, :K.max()], K))
    p0 = pick_p0(_p0(c0, c1), p0)
    T = max(p[0].shape[1] for p in per)
    cx = np.zeros((R, T), np.int64)
    bt = np.zeros((R, T), np.int64)
    K = np.concatenate([p[2] for p in per])
    for k, (a, b, _) in enumerate(per):
        cx[k * LANES:(k + 1) * LANES, :a.shape[1]] = a
        bt[k * LANES:(k + 1) * LANES, :b.shape[1]] = b
    lanes = np.arange(R)
    model = np.tile(p0, (R, 1))
    prob = np.zeros_like(cx)
    for t in range(T):
        act = t < K
        p = model[lanes, cx[:, t]]
        prob[:, t] = p
        model[lanes[act], cx[act, t]] = _adapt(p, bt[:, t])[act]
    x = np.full(R, L, np.int64)
    words = np.zeros((R, T), np.int64)
    cnt = np.zeros(R, np.int64)
    for t in range(T - 1, -1, -1):
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
        run = [int(w) for l in ls for w in words[l, :cnt[l]][::-1]]
        chunks.append(st + [int(cnt[l]) for l in ls] + run)
    body = struct.pack("<16I", *cells) + struct.pack("<II", S, nc) + struct.pack("<%dH" % nctx, *p0.tolist())
    body += b"".join(struct.pack("<I", len(ch)) for ch in chunks)
    body += b"".join(struct.pack("<%dH" % len(ch), *ch) for ch in chunks)
    return head + struct.pack("<I", len(body)) + body


def _header(blob, any_layout=False):
    assert len(blob) >= HEAD and blob[0] == ord("A") and blob[1] == 2, "not an attribute blob of version 2"
    bpv, slod, c = blob[2] & 15, blob[2] >> 4, blob[3]
    assert bpv in (1, 2) and 1 <= c <= 4
    n, plen = struct.unpack_from("<II", blob, 4)
    if n == 0:
        assert plen == 0
        return bpv, c, 0, None
    assert len(blob) >= HEAD2 + 2 * contexts(bpv, c), "truncated header"
    cells = struct.unpack_from("<16I", blob, HEAD)
    S, nc = struct.unpack_from("<II", blob, HEAD + 64)
    assert cells[0] == n and all(b <= a and 8 * b >= a for a, b in zip(cells, cells[1:])) and cells[15] >= 1
    if any_layout:
        check_layout(n, c, S, nc)
    else:
        assert (S, nc) == layout(n, c)
    off_table = HEAD2 + 2 * contexts(bpv, c)
    assert len(blob) >= off_table + 4 * nc, "truncated chunk table"
    words = struct.unpack_from("<%dI" % nc, blob, off_table)
    assert off_table + 4 * nc + 2 * sum(words) == HEAD + plen
    return bpv, c, n, (cells, S, nc, words, off_table + 4 * nc, slod)


def lod_info(blob, lod, any_layout=False):
    """(bytes, values): blob[:bytes] is the shortest prefix that decodes at `lod`; `blob` may be a prefix that reaches
    the last needed chunk's length table"""
    assert 0 <= lod <= 15
    bpv, c, n, h = _header(blob, any_layout)
    if n == 0:
        return HEAD, 0
    cells, S, nc, words, off_payload, _ = h
    if lod == 0:
        return off_payload + 2 * sum(words), n
    m = cells[lod]
    lanes = -(-m // S)
    cs, ls = (lanes - 1) // LANES, (lanes - 1) % LANES
    start = off_payload + 2 * sum(words[:cs])
    assert len(blob) >= start + 2 * 192, "truncated in front of the length table"
    lens = np.frombuffer(blob, "<u2", LANES, start + 2 * 128)
    run = 192 + int(lens[:ls + 1].sum())
    assert run <= words[cs]
    return start + 2 * run, m


def _residuals(blob, m, any_layout=False):
    """the first m residuals [m, c] of the introduction sequence from the bytes lod_info names"""
    out, bpv, bad = _lanes(blob, m, any_layout, True, False)
    assert bad == 0
    return out, bpv


def status(blob, m, any_layout=False, whole=None):
    """the status word the lane decoder leaves for the first m values of this frame, bits as attr_ref.status states
    them; a lane whose run the level cuts short is exempt from the checks at its end.  whole: the last needed chunk is
    there with all its words, as at lod 0 (the default when m is every value of the blob), not only up to the last
    needed lane's run"""
    n = struct.unpack_from("<I", blob, 4)[0]
    return _lanes(blob, m, any_layout, False, m == n if whole is None else whole)[2]


def _lanes(blob, m, any_layout, strict, whole_last):
    """-> (residuals, bpv, status); strict: a stream that would set a status bit stops at an assert instead"""
    bpv, c, n, (cells, S, nc, words, at, _) = _header(blob, any_layout)
    nctx, P, kmax = contexts(bpv, c), positions(bpv), 8 * bpv - 1
    p0 = np.array(struct.unpack_from("<%dH" % nctx, blob, HEAD2), np.int64)
    assert ((p0 >= 16) & (p0 <= 4080)).all()
    lanes_needed = -(-m // S)
    out = np.zeros((nc * LANES * S, c), np.int64)
    lanes = np.arange(LANES)
    bad = 0
    for k in range(-(-lanes_needed // LANES)):
        full = np.clip(n - (k * LANES + lanes) * S, 0, S)                # the lane's run in the whole blob
        npts = np.clip(m - (k * LANES + lanes) * S, 0, S)                # what this level takes of it
        last = int(np.nonzero(npts > 0)[0].max())
        assert len(blob) >= at + 2 * 192, "truncated"
        hw = np.frombuffer(blob, "<u2", 192, at).astype(np.int64)
        x = hw[0:128:2] | (hw[1:128:2] << 16)
        ln = hw[128:192]
        assert not strict or 192 + ln.sum() == words[k]
        have = 192 + int(ln[:last + 1].sum())
        if whole_last or k + 1 < -(-lanes_needed // LANES):
            have = words[k]
        if 192 + ln.sum() != words[k]:
            bad |= 1
            at += 2 * words[k]
            continue
        assert len(blob) >= at + 2 * have, "truncated"
        w = np.frombuffer(blob, "<u2", have, at).astype(np.int64)
        at += 2 * words[k]
        pos = 192 + np.concatenate([[0], np.cumsum(ln)[:-1]])
        end = pos + ln
        model = np.tile(p0, (LANES, 1))
        s, chn, phase, i, acc, neg = (np.zeros(LANES, np.int64) for _ in range(6))
        bk = np.zeros((LANES, c), np.int64)
        while (s < npts).any():
            act = s < npts
            cpos = np.select([phase == 0, phase == 1, phase == 2], [0, 1, 2 + i], 1 + kmax + i)
            ctx = np.where(act, (chn * BUCKETS + bk[lanes, chn]) * P + cpos, 0)
            p1 = model[lanes, ctx]
            cum = x & 4095
            bit = (cum >= 4096 - p1).astype(np.int64)
            freq = np.where(bit == 1, p1, 4096 - p1)
            x = np.where(act, freq * (x >> 12) + cum - np.where(bit == 1, 4096 - p1, 0), x)
            model[lanes[act], ctx[act]] = _adapt(p1, bit)[act]
            need = act & (x < L)
            assert not strict or not (need & (pos >= end)).any(), "a lane ran out of words"
            bad |= 1 if (need & (pos >= end)).any() else 0
            x = np.where(need, (x << 16) | w[np.minimum(pos, have - 1)], x)
            pos += need
            ph0, ph1, ph2, ph3 = phase == 0, phase == 1, phase == 2, phase == 3
            kk = i + bit
            end2 = ph2 & ((bit == 0) | (kk == kmax))
            done = (ph0 & (bit == 0)) | (end2 & (kk == 0)) | (ph3 & (i == 1))
            mag = np.where(ph3, 2 * acc + bit, np.where(end2 & (kk == 0), 1, 0))
            neg = np.where(ph1, bit, neg)
            phase, i, acc = (np.select([ph0, ph1, end2, ph2], [1, 2, 3, 2], 3),
                             np.select([ph1, end2, ph2, ph3], [0, kk, kk, i - 1], i),
                             np.select([end2, ph3], [1, 2 * acc + bit], acc))
            fin = act & done
            fl, fc = lanes[fin], chn[fin]
            out[((k * LANES + lanes) * S + s)[fin], fc] = np.where(neg == 1, -mag, mag)[fin]
            bk[fl, fc] = _bucket(mag[fin])
            phase = np.where(fin, 0, phase)
            neg = np.where(fin, 0, neg)
            chn = np.where(fin, chn + 1, chn)
            s = np.where(fin & (chn == c), s + 1, s)
            chn = np.where(chn == c, 0, chn)
        whole = npts == full                                             # lanes whose run this level takes entirely
        assert not strict or ((pos == end)[whole].all() and (x == L)[whole].all()), "corrupt chunk"
        bad |= (0 if (pos == end)[whole].all() else 1) | (0 if (x == L)[whole].all() else 4)
    return out[:m], bpv, bad


def decode(blob, cells, lod=0, any_layout=False):
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    bpv, c, n, h = _header(blob, any_layout)
    m = cells.shape[0]
    if n == 0:
        assert m == 0
        return np.zeros((0, c), np.int64), bpv
    assert m == h[0][lod], "the blob has %d values at lod %d, the geometry %d cells" % (h[0][lod], lod, m)
    assert len(blob) >= lod_info(blob, lod, any_layout)[0], "truncated"
    r, _ = _residuals(blob, m, any_layout)
    assert h[5] + lod <= 15
    keys = np.sort(keys_of(cells, 32768 >> (h[5] + lod)))
    s, order, first = intro(keys)
    assert [int((s >= j).sum()) for j in range(16 - lod)] == list(h[0][lod:]), "the cells do not give the header's counts"
    mask = (1 << (8 * bpv)) - 1
    val = np.zeros((m, c), np.int64)
    res = np.zeros((m, c), np.int64)
    res[order] = r                                                      # residual of every Morton index
    val[0] = res[0] & mask
    for size in range(15, -1, -1):                                      # a size's predictors are all coarser: done
        at = np.nonzero((s == size) & (np.arange(m) > 0))[0]
        val[at] = (val[first[at]] + res[at]) & mask
    return val, bpv
