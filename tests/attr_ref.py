"""A second statement of attribute blob version 1 (the layout in csrc/attr.hip's header), written from that description
in numpy: a value's binarisation as 16 bpv fixed slots with a validity mask, and the models and rANS states of all lanes
stepped side by side.  Not a port of the kernels, which walk one lane's values with a loop per decision.

    encode(values, bpv)              -> blob                          values int [n] or [n, c]
                                        layout=(S, n_chunks): any layout the parser accepts (check_layout) in place
                                        of layout(n, c); p0=: the initial table, nctx entries or one for all, in
                                        place of the counted one.  The coding is the same for every layout and table
    decode(blob)                     -> (values int64 [n, c], bpv)
    status(blob)                     -> the decoder's status word of the frame (csrc/attr.hip, above ADFrame): the
                                        OR over chunks and lanes of 1 = words, 4 = final state; 0 for a sound blob
    single_stream_bytes(values, bpv) -> bytes of the frame as ONE lane: same model, same p0, one final state (the
                                        ideal code length of its decisions rounded up to words, its 4-byte state and
                                        the one-chunk header)
    merge(points, values)            -> the codec's duplicate rule
"""
import math
import struct

import numpy as np

HEAD = 12
BUCKETS = 5
MAX_VALUES = 512
LANES = 64
L = 1 << 16


def positions(bpv):
    return 16 * bpv


def contexts(bpv, c):
    return c * BUCKETS * positions(bpv)


def layout(n, c):
    """(S, chunks): as few chunks as 512 values per lane allow, the points spread evenly over their lanes"""
    smax = MAX_VALUES // c
    k = max(1, -(-n // (LANES * smax)))
    return max(1, -(-n // (LANES * k))), k


def check_layout(n, c, S, nc):
    """the four conditions under which the parsers of csrc/attr_blob.h take (S, chunks) for n > 0 points of c channels"""
    assert S >= 1, (S, nc)
    assert S * c <= MAX_VALUES, (S, c)
    assert 1 <= nc <= n, (nc, n)
    assert LANES * S * (nc - 1) < n <= LANES * S * nc, (n, S, nc)


def pick_layout(n, c, given=None):
    """layout(n, c), or the (S, chunks) given if the parsers take it"""
    if given is None:
        return layout(n, c)
    S, nc = (int(a) for a in given)
    check_layout(n, c, S, nc)
    return S, nc


def pick_p0(counted, given=None):
    """the counted table, or the one given: an entry per context or one for all, each in [16, 4080]"""
    if given is None:
        return counted
    p0 = np.broadcast_to(np.asarray(given, np.int64), counted.shape).copy()
    assert ((p0 >= 16) & (p0 <= 4080)).all()
    return p0


def _bucket(m):
    return (m >= 2).astype(np.int64) + (m >= 5) + (m >= 12) + (m >= 30)


def _resid(runs, bpv):
    """runs int64 [R, S, c] -> residuals r and the bucket of the channel's previous residual in the run"""
    S = runs.shape[1]
    kmax = 8 * bpv - 1
    half, mask = 1 << kmax, (1 << (8 * bpv)) - 1
    a = np.zeros_like(runs)
    b = np.zeros_like(runs)
    a[:, 1:] = runs[:, :-1]
    b[:, 2:] = runs[:, :-2]
    pred = np.where((np.arange(S) == 1)[None, :, None], a, (a + b + 1) >> 1)
    pred[:, 0] = 0
    r = ((runs - pred + half) & mask) - half
    bk = np.zeros_like(runs)
    bk[:, 1:] = _bucket(np.abs(r[:, :-1]))
    return r, bk


def _slots(r, bk, valid, bpv):
    """r, bk [R, S, c], valid bool [R, S] -> ctx, bit, ok [R, S c P]: every run's decisions in coding order, the slots
    that are not coded masked"""
    R, S, c = r.shape
    kmax, P = 8 * bpv - 1, positions(bpv)
    m = np.abs(r)
    k = np.zeros_like(m)
    nz = m > 0
    k[nz] = np.floor(np.log2(m[nz])).astype(np.int64)
    base = (np.arange(c)[None, None, :] * BUCKETS + bk) * P
    ctx = np.zeros((R, S, c, P), np.int32)
    bit = np.zeros((R, S, c, P), np.int8)
    ok = np.zeros((R, S, c, P), bool)
    ctx[..., 0], bit[..., 0], ok[..., 0] = base, nz, True                       # zero flag
    ctx[..., 1], bit[..., 1], ok[..., 1] = base + 1, r < 0, nz                  # sign
    for i in range(kmax):                                                        # prefix: k ones, a zero below kmax
        ctx[..., 2 + i], bit[..., 2 + i], ok[..., 2 + i] = base + 2 + i, i < k, nz & (i <= k)
    for q in range(kmax):                                                        # suffix: bits k-1 .. 0 of m
        j = np.maximum(k - 1 - q, 0)
        ctx[..., 2 + kmax + q], bit[..., 2 + kmax + q], ok[..., 2 + kmax + q] = base + 2 + kmax + j, (m >> j) & 1, nz & (q < k)
    ok &= valid[:, :, None, None]
    return ctx.reshape(R, -1), bit.reshape(R, -1), ok.reshape(R, -1)


def _p0(c0, c1):
    return np.clip((4096 * (2 * c1 + 1)) // (2 * (c0 + c1 + 1)), 16, 4080)


def _adapt(p, bit):
    return np.where(bit == 1, p + ((4096 - p) >> 4), p - (p >> 4))


def _as2d(values):
    v = np.asarray(values).astype(np.int64)
    return v[:, None] if v.ndim == 1 else v


def encode(values, bpv, layout=None, p0=None):
    v = _as2d(values)
    n, c = v.shape
    head = bytes([ord("A"), 1, bpv, c]) + struct.pack("<I", n)
    if n == 0:
        return head + struct.pack("<I", 0)
    S, nc = pick_layout(n, c, layout)
    R = nc * LANES
    runs = np.zeros((R * S, c), np.int64)
    runs[:n] = v
    runs = runs.reshape(R, S, c)
    valid = (np.arange(R * S) < n).reshape(R, S)
    r, bk = _resid(runs, bpv)
    nctx = contexts(bpv, c)
    # a chunk's 64 runs at a time: the counting pass, and every run's coded decisions first (stable)
    c0 = np.zeros(nctx, np.int64)
    c1 = np.zeros(nctx, np.int64)
    per = []
    for k in range(nc):
        sl = slice(k * LANES, (k + 1) * LANES)
        ctx, bit, ok = _slots(r[sl], bk[sl], valid[sl], bpv)
        c1 += np.bincount(ctx[ok & (bit == 1)], minlength=nctx)
        c0 += np.bincount(ctx[ok & (bit == 0)], minlength=nctx)
        order = np.argsort(~ok, axis=1, kind="stable")
        K = ok.sum(1)
        per.append((np.take_along_axis(ctx, order, 1)[:, :K.max()], np.take_along_axis(bit, order, 1)[:, :K.max()], K))
    p0 = pick_p0(_p0(c0, c1), p0)
    T = max(p[0].shape[1] for p in per)
    cx = np.zeros((R, T), np.int64)
    bt = np.zeros((R, T), np.int64)
    K = np.concatenate([p[2] for p in per])
    for k, (a, b, _) in enumerate(per):
        cx[k * LANES:(k + 1) * LANES, :a.shape[1]] = a
        bt[k * LANES:(k + 1) * LANES, :b.shape[1]] = b
    lanes = np.arange(R)
    # forward: every lane's model from p0 -> the probability of a one in front of each decision
    model = np.tile(p0, (R, 1))
    prob = np.zeros_like(cx)
    for t in range(T):
        act = t < K
        p = model[lanes, cx[:, t]]
        prob[:, t] = p
        model[lanes[act], cx[act, t]] = _adapt(p, bt[:, t])[act]
    # backward: rANS over each lane's decisions in reverse, L = 2^16, 16-bit words, 12-bit probabilities
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
        run = [int(w) for l in ls for w in words[l, :cnt[l]][::-1]]              # the order the decoder takes them
        chunks.append(st + [int(cnt[l]) for l in ls] + run)
    body = struct.pack("<II", S, nc) + struct.pack("<%dH" % nctx, *p0.tolist())
    body += b"".join(struct.pack("<I", len(ch)) for ch in chunks)
    body += b"".join(struct.pack("<%dH" % len(ch), *ch) for ch in chunks)
    return head + struct.pack("<I", len(body)) + body


def decode(blob):
    """blob -> (values int64 [n, c], bpv): every lane a state machine over its binarisation, all 64 lanes of a chunk
    stepped together"""
    out, bpv, bad = _decode(blob, True)
    assert bad == 0
    return out, bpv


def status(blob):
    """the status word the lane decoder leaves for this frame: bit 1 = a chunk whose 192 + sum of len is not its table
    entry (it is then not decoded), a lane that needs a word at or behind the end of its run (it goes on with the
    chunk's words by position, the last of them again and again), a lane that ends in front of the end of its run;
    bit 4 = a lane that does not end in the state 2^16"""
    return _decode(blob, False)[2]


def _decode(blob, strict):
    """-> (values, bpv, status); strict: a stream that would set a status bit stops at an assert instead"""
    tag, ver, bpv, c = blob[0], blob[1], blob[2], blob[3]
    assert tag == ord("A") and ver == 1 and bpv in (1, 2) and 1 <= c <= 4
    n, plen = struct.unpack_from("<II", blob, 4)
    assert HEAD + plen == len(blob)
    if n == 0:
        return np.zeros((0, c), np.int64), bpv, 0
    S, nc = struct.unpack_from("<II", blob, HEAD)
    check_layout(n, c, S, nc)
    nctx, P, kmax = contexts(bpv, c), positions(bpv), 8 * bpv - 1
    mask = (1 << (8 * bpv)) - 1
    at = HEAD + 8
    p0 = np.array(struct.unpack_from("<%dH" % nctx, blob, at), np.int64)
    at += 2 * nctx
    cw = struct.unpack_from("<%dI" % nc, blob, at)
    at += 4 * nc
    out = np.zeros((nc * LANES * S, c), np.int64)
    lanes = np.arange(LANES)
    bad = 0
    for k in range(nc):
        w = np.array(struct.unpack_from("<%dH" % cw[k], blob, at), np.int64)
        at += 2 * cw[k]
        x = w[0:128:2] | (w[1:128:2] << 16)
        ln = w[128:192]
        assert not strict or 192 + ln.sum() == cw[k]
        if 192 + ln.sum() != cw[k]:
            bad |= 1
            continue
        pos = 192 + np.concatenate([[0], np.cumsum(ln)[:-1]])
        end = pos + ln
        npts = np.clip(n - (k * LANES + lanes) * S, 0, S)
        model = np.tile(p0, (LANES, 1))
        s, chn, phase, i, acc, neg = (np.zeros(LANES, np.int64) for _ in range(6))
        bk, v1, v2 = (np.zeros((LANES, c), np.int64) for _ in range(3))
        while (s < npts).any():
            act = s < npts
            cpos = np.select([phase == 0, phase == 1, phase == 2], [0, 1, 2 + i], 1 + kmax + i)
            ctx = np.where(act, (chn * BUCKETS + bk[lanes, chn]) * P + cpos, 0)   # lanes that are done: any context
            p1 = model[lanes, ctx]
            cum = x & 4095
            bit = (cum >= 4096 - p1).astype(np.int64)
            freq = np.where(bit == 1, p1, 4096 - p1)
            x = np.where(act, freq * (x >> 12) + cum - np.where(bit == 1, 4096 - p1, 0), x)
            model[lanes[act], ctx[act]] = _adapt(p1, bit)[act]
            need = act & (x < L)
            assert not strict or not (need & (pos >= end)).any(), "a lane ran out of words"
            bad |= 1 if (need & (pos >= end)).any() else 0
            x = np.where(need, (x << 16) | w[np.minimum(pos, cw[k] - 1)], x)
            pos += need
            # the next place in the binarisation; done = the value is complete, m its magnitude
            ph0, ph1, ph2, ph3 = phase == 0, phase == 1, phase == 2, phase == 3
            kk = i + bit
            end2 = ph2 & ((bit == 0) | (kk == kmax))
            done = (ph0 & (bit == 0)) | (end2 & (kk == 0)) | (ph3 & (i == 1))
            m = np.where(ph3, 2 * acc + bit, np.where(end2 & (kk == 0), 1, 0))
            neg = np.where(ph1, bit, neg)
            phase, i, acc = (np.select([ph0, ph1, end2, ph2], [1, 2, 3, 2], 3),
                             np.select([ph1, end2, ph2, ph3], [0, kk, kk, i - 1], i),
                             np.select([end2, ph3], [1, 2 * acc + bit], acc))
            fin = act & done
            a, b = v1[lanes, chn], v2[lanes, chn]
            pred = np.where(s == 0, 0, np.where(s == 1, a, (a + b + 1) >> 1))
            val = (pred + np.where(neg == 1, -m, m)) & mask
            fl, fc = lanes[fin], chn[fin]
            out[((k * LANES + lanes) * S + s)[fin], fc] = val[fin]
            v2[fl, fc] = a[fin]
            v1[fl, fc] = val[fin]
            bk[fl, fc] = _bucket(m[fin])
            phase = np.where(fin, 0, phase)
            neg = np.where(fin, 0, neg)
            chn = np.where(fin, chn + 1, chn)
            s = np.where(fin & (chn == c), s + 1, s)
            chn = np.where(chn == c, 0, chn)
        assert not strict or ((pos == end).all() and (x == L).all()), "corrupt chunk"
        bad |= (0 if (pos == end).all() else 1) | (0 if (x == L).all() else 4)
    return out[:n], bpv, bad


def single_stream_bytes(values, bpv):
    v = _as2d(values)
    n, c = v.shape
    r, bk = _resid(v[None], bpv)
    nctx = contexts(bpv, c)
    cxs, bts = [], []
    blk = 1 << 15
    for lo in range(0, n, blk):                           # the slots a block of points at a time (memory)
        ctx, bit, ok = _slots(r[:, lo:lo + blk], bk[:, lo:lo + blk], np.ones((1, min(blk, n - lo)), bool), bpv)
        cxs.append(ctx[ok])
        bts.append(bit[ok])
    ctx, bit = np.concatenate(cxs), np.concatenate(bts).astype(np.int64)
    p0 = _p0(np.bincount(ctx[bit == 0], minlength=nctx), np.bincount(ctx[bit == 1], minlength=nctx))
    model = p0.tolist()
    cost = [0.0] + [math.log2(4096.0 / f) for f in range(1, 4097)]
    bits = 0.0
    for cx, b in zip(ctx.tolist(), bit.tolist()):
        p = model[cx]
        if b:
            bits += cost[p]
            model[cx] = p + ((4096 - p) >> 4)
        else:
            bits += cost[4096 - p]
            model[cx] = p - (p >> 4)
    return HEAD + 8 + 2 * nctx + 4 + 4 + 2 * math.ceil(bits / 16)


def merge(points, values):
    """unique rows of points (np.unique order) and per row the rounded mean (sum + cnt // 2) // cnt of its
    duplicates' values"""
    v = _as2d(values)
    u, inv, cnt = np.unique(np.asarray(points), axis=0, return_inverse=True, return_counts=True)
    sums = np.zeros((u.shape[0], v.shape[1]), np.int64)
    np.add.at(sums, inv.reshape(-1), v)
    return u, (sums + cnt[:, None] // 2) // cnt[:, None]
