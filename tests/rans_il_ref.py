"""Plain numpy restatement of the wave-interleaved rANS stream of container version 1 (the layout, the coding step and
the order of the rounds are the ones stated at the top of csrc/rans_gpu.hip and in oracle/pcc_oracle.c), for the things
the C oracle cannot do: a forced number of steps per chunk T, and damaged streams (a forced escape count nibble).

    stream  = u32 'PCI2' | u32 n | u32 T | u32 n_chunks | u32 words[n_chunks] | chunk payloads (16-bit words)
    chunk c = symbols [c 64 T, (c+1) 64 T): step t of lane l codes symbol c 64 T + 64 t + l
    payload = 64 x (state lo, state hi) | block(step 0, round 0) | block(0, 1) .. | block(1, 0) ..

Integer division, one state per lane, vectorised over the 64 lanes only.  `tables` is (cdf [R, pitch], sizes [R],
offsets [R]) as the coders take them.  Below the coder: the edge table set both test files use, and ctypes wrappers of
the oracle's orc_rans_interleaved_* for arbitrary tables (oracle/codec_ref.py binds them to the model's tables only)."""
import ctypes as C
import struct

import numpy as np

LANES = 64
MAGIC = 0x32494350   # "PCI2"
L = 1 << 16


class StreamError(ValueError):
    """code: the oracle decoder's -1 (header), -2 (a chunk out of words / length), -3 (nibble count above 8)"""

    def __init__(self, code, text):
        super().__init__(f"interleaved rANS stream: {text} ({code})")
        self.code = code


def steps_for(n):
    return 320 if n > 262144 else 80 if n > 32768 else max((n + LANES - 1) // LANES, 1)


def chunks_for(n, T):
    return max(-(-n // (LANES * T)), 1)


def _rows(idx, n, idx_run):
    if idx is not None:
        return np.ascontiguousarray(idx, dtype=np.uint8).reshape(-1).astype(np.int64)
    return np.arange(n, dtype=np.int64) // idx_run


def lookup(sym, rows, tables):
    """per symbol: start, freq of its bin, raw escape value, nibbles of raw, escaped or not (all int64 / bool)"""
    cdf, sizes, offsets = (np.asarray(a, dtype=np.int64) for a in tables)
    maxv = sizes[rows] - 2
    v0 = np.asarray(sym, dtype=np.int64) - offsets[rows]
    assert v0.size == 0 or (v0.min() >= -2 ** 31 and v0.max() < 2 ** 31), "the coder's domain: sym - offset fits int32"
    neg, big = v0 < 0, v0 >= maxv
    raw = np.where(neg, -2 * v0 - 1, np.where(big, 2 * (v0 - maxv), 0))
    esc = neg | big
    v = np.where(esc, maxv, v0)
    nb = np.zeros(raw.shape, dtype=np.int64)
    for k in range(8):
        nb += (raw >> (4 * k)) != 0
    start = cdf[rows, v]
    return start, cdf[rows, v + 1] - start, raw, nb, esc


def encode(sym, idx, tables, idx_run=1, T=None, nibble_count=None, trace=None):
    """bytes of the stream.  T=None: the encoder's rule; a forced T writes the chunk count that goes with it.
    nibble_count: {symbol position: count nibble written in place of the true one} (the symbol must escape).
    trace(x, freq): called with the states and frequencies of every division (round 0 of a step, the live lanes)"""
    sym = np.ascontiguousarray(sym, dtype=np.int32).reshape(-1)
    n = sym.shape[0]
    T = steps_for(n) if T is None else int(T)
    nc = chunks_for(n, T)
    start, freq, raw, nb, esc = lookup(sym, _rows(idx, n, idx_run), tables)
    cnt_nib = nb.copy()
    for pos, val in (nibble_count or {}).items():
        assert esc[pos], "a forced count nibble needs a symbol that escapes"
        cnt_nib[pos] = val
    pad = nc * LANES * T - n
    act = np.concatenate([np.ones(n, dtype=bool), np.zeros(pad, dtype=bool)]).reshape(nc, T, LANES)

    def shaped(a, fill):
        return np.concatenate([a, np.full(pad, fill, dtype=a.dtype)]).reshape(nc, T, LANES)
    start, freq, raw, nb, cnt_nib, esc = (shaped(a, f) for a, f in ((start, 0), (freq, 1), (raw, 0), (nb, 0), (cnt_nib, 0),
                                                                    (esc, False)))
    words, payloads = [], []
    for c in range(nc):
        x = np.full(LANES, L, dtype=np.int64)
        blocks = []                                   # in coding order: the stream holds them reversed
        for t in range(T - 1, -1, -1):
            a, e, k = act[c, t], esc[c, t], nb[c, t]
            if not a.any():
                continue
            if e.any():
                for r in range(9, 0, -1):             # bypass rounds, last first: 1 = nibble count, 2 + j = nibble j
                    m = e & (r <= 1 + k)
                    if not m.any():
                        continue
                    need = m & (x >= (1 << 28))
                    blocks.append(x[need] & 0xFFFF)
                    x[need] >>= 16
                    val = cnt_nib[c, t] if r == 1 else (raw[c, t] >> (4 * (r - 2))) & 15
                    x[m] = (x[m] << 4) | val[m]
            f = freq[c, t]
            need = a & (x >= (f << 16))
            blocks.append(x[need] & 0xFFFF)
            x[need] >>= 16
            if trace is not None:
                trace(x[a], f[a])
            x[a] = ((x[a] // f[a]) << 16) + x[a] % f[a] + start[c, t][a]
        states = np.stack([x & 0xFFFF, x >> 16], axis=1).reshape(-1)
        p = np.concatenate([states] + blocks[::-1]).astype(np.uint16)
        words.append(p.shape[0])
        payloads.append(p.tobytes())
    return struct.pack("<4I", MAGIC, n, T, nc) + np.asarray(words, dtype=np.uint32).tobytes() + b"".join(payloads)


def quotient_f32(x, f):
    """k_rans_enc's division in numpy: (q0, q, rem) — q0 from one float32 multiplication by 1 / freq, then the kernel's
    32-bit under / over correction"""
    x, f = np.asarray(x).astype(np.uint32), np.asarray(f).astype(np.uint32)
    q0 = (x.astype(np.float32) * (np.float32(1) / f.astype(np.float32))).astype(np.uint32)
    fi = f.view(np.int32)
    r0 = (x - q0 * f).view(np.int32)                                  # wraps like the kernel's 32-bit arithmetic
    under, over = r0 < 0, r0 >= fi
    qd = q0 - under.astype(np.uint32) + over.astype(np.uint32)
    rem = r0 + np.where(under, fi, 0).astype(np.int32) - np.where(over, fi, 0).astype(np.int32)
    return q0, qd, rem.view(np.uint32)


def header(data):
    """(n, T, words of every chunk) of a stream"""
    magic, n, T, nc = struct.unpack_from("<4I", data, 0)
    assert magic == MAGIC
    return n, T, np.frombuffer(data, dtype=np.uint32, count=nc, offset=16).astype(np.int64)


def decode(data, idx, n, tables, idx_run=1):
    """int32 [n]; raises StreamError with the oracle decoder's code"""
    cdf, sizes, offsets = (np.asarray(a, dtype=np.int64) for a in tables)
    if len(data) < 16:
        raise StreamError(-1, "shorter than its header")
    magic, hn, T, nc = struct.unpack_from("<4I", data, 0)
    if magic != MAGIC or hn != n or T < 1 or nc < 1 or len(data) < 4 * (4 + nc) or LANES * T * nc < n:
        raise StreamError(-1, "bad header")
    cw_all = np.frombuffer(data, dtype=np.uint32, count=nc, offset=16).astype(np.int64)
    w16 = np.frombuffer(data, dtype=np.uint16, offset=4 * (4 + nc), count=(len(data) - 4 * (4 + nc)) // 2).astype(np.int64)
    rows_all = _rows(idx, n, idx_run)
    # entries past a row's length never compare <= a cumulative count
    cdfp = np.where(np.arange(cdf.shape[1])[None, :] < sizes[:, None], cdf, 1 << 20)
    out = np.zeros(n, dtype=np.int64)
    lanes = np.arange(LANES)
    pos = 0
    for c in range(nc):
        cw = int(cw_all[c])
        if cw < 2 * LANES or 4 * (4 + nc) + (pos + cw) * 2 > len(data):
            raise StreamError(-2, f"chunk {c} has no states or leaves the stream")
        p = w16[pos:pos + cw]
        x = p[0:2 * LANES:2] | (p[1:2 * LANES:2] << 16)
        ptr = 2 * LANES

        def refill(need):
            nonlocal ptr
            cnt = int(need.sum())
            if ptr + cnt > cw:
                raise StreamError(-2, f"chunk {c} ran out of words")
            x[need] = (x[need] << 16) | p[ptr:ptr + cnt]
            ptr += cnt

        for t in range(T):
            i = c * LANES * T + t * LANES + lanes
            a = i < n
            if not a.any():
                continue
            r = rows_all[i[a]]
            xa = x[a]
            cum = xa & 0xFFFF
            s = (cdfp[r, 1:] <= cum[:, None]).sum(axis=1)
            c0 = cdf[r, s]
            x[a] = (cdf[r, s + 1] - c0) * (xa >> 16) + cum - c0
            maxv = np.zeros(LANES, dtype=np.int64)
            value = np.zeros(LANES, dtype=np.int64)
            maxv[a], value[a] = sizes[r] - 2, s
            esc = a & (value == maxv)
            refill(a & (x < L))
            if esc.any():
                active = esc.copy()
                remaining = np.full(LANES, -1)
                j = np.zeros(LANES, dtype=np.int64)
                raw = np.zeros(LANES, dtype=np.int64)
                while active.any():
                    val = x & 15
                    x[active] >>= 4
                    refill(active & (x < L))
                    first = active & (remaining < 0)
                    if (val[first] > 8).any():
                        raise StreamError(-3, "a nibble count above 8")
                    rest = active & ~first
                    raw[rest] |= val[rest] << (4 * j[rest])
                    j[rest] += 1
                    remaining[rest] -= 1
                    remaining[first] = val[first]
                    active &= remaining != 0
                ev = raw >> 1
                value = np.where(esc, np.where(raw & 1, -ev - 1, ev + maxv), value)
            v = value[a] + offsets[r]
            out[i[a]] = ((v + 2 ** 31) % 2 ** 32) - 2 ** 31    # int32 arithmetic, like the coders
        pos += cw
    if 4 * (4 + nc) + pos * 2 != len(data):
        raise StreamError(-2, "bytes behind the last chunk")
    return out.astype(np.int32)


# ---------------------------------------------------------------------------------- the oracle on arbitrary tables
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _c_tables(tables):
    return tuple(np.ascontiguousarray(a, dtype=np.int32) for a in tables)


def oracle_encode(oracle, sym, idx, tables, idx_run=1):
    cdf, sizes, offs = _c_tables(tables)
    sym = np.ascontiguousarray(sym, dtype=np.int32).reshape(-1)
    n = sym.shape[0]
    idx8 = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint8).reshape(-1)
    cap = 48 * n + 4096
    out = np.empty(cap, dtype=np.uint8)
    oracle.lib.orc_rans_interleaved_encode.restype = C.c_int64
    got = oracle.lib.orc_rans_interleaved_encode(_p(sym), _p(idx8) if idx8 is not None else None, C.c_int64(idx_run),
                                                 C.c_int64(n), _p(cdf), C.c_int(cdf.shape[1]), _p(sizes), _p(offs), _p(out),
                                                 C.c_int64(cap))
    assert got >= 0
    return out[:got].tobytes()


def oracle_decode_rc(oracle, data, idx, n, tables, idx_run=1):
    """(return code, symbols): 0, or the oracle decoder's negative code"""
    cdf, sizes, offs = _c_tables(tables)
    idx8 = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint8).reshape(-1)
    buf = np.frombuffer(data, dtype=np.uint8)
    sym = np.zeros(n, dtype=np.int32)
    oracle.lib.orc_rans_interleaved_decode.restype = C.c_int
    rc = oracle.lib.orc_rans_interleaved_decode(_p(buf), C.c_int64(buf.shape[0]), _p(idx8) if idx8 is not None else None,
                                                C.c_int64(idx_run), C.c_int64(n), _p(cdf), C.c_int(cdf.shape[1]),
                                                _p(sizes), _p(offs), _p(sym))
    return rc, sym


# ---------------------------------------------------------------------------------- the edge table set
ROW_A, ROW_B, ROW_C, ROW_D = 0, 1, 2, 3
SWEEP_FREQS = sorted({1, 2, 3, 5, 7} | {(1 << k) + d for k in range(2, 16) for d in (-1, 0, 1)})
ESCAPE_RAWS = [0, 1] + [v for k in range(1, 8) for v in (16 ** k - 1, 16 ** k)] + [2 ** 32 - 1]   # counts 0..8


def tables_of(rows, offsets):
    """(cdf, sizes, offsets) from a list of CDFs of different lengths"""
    pitch = max(len(r) for r in rows)
    cdf = np.zeros((len(rows), pitch), dtype=np.int32)
    for i, r in enumerate(rows):
        cdf[i, :len(r)] = r
    return cdf, np.asarray([len(r) for r in rows], dtype=np.int32), np.asarray(offsets, dtype=np.int32)


def sweep_rows():
    """CDFs whose bins run through SWEEP_FREQS in shuffled order, one fill bin making each sum 65536 and an escape bin
    of frequency 1.  The frequencies add up to 196599, so they take four rows (first fit), not two."""
    rng = np.random.default_rng(4)
    freqs = [int(f) for f in rng.permutation(SWEEP_FREQS)]
    bins = []
    for f in freqs:
        for b in bins:
            if sum(b) + f <= 65535:
                b.append(f)
                break
        else:
            bins.append([f])
    rows = []
    for b in bins:
        fill = 65535 - sum(b)
        if fill:
            b.insert(int(rng.integers(0, len(b) + 1)), fill)
        rows.append(np.concatenate([[0], np.cumsum(b + [1])]))
        assert rows[-1][-1] == 65536
    return rows


def edge_tables():
    """A: only the escape bin.  B: 1000 bins of frequency 1 in LUT bucket 0, one bin across 63 buckets, escape bin of
    frequency 1.  C: every edge on a bucket edge.  D: one near-certain bin, escape bin of frequency 1.  E..: the
    frequency sweep.  Offsets 0 on A and D, positive elsewhere (so that every raw escape value fits on every row)."""
    rows = [np.array([0, 65536]), np.concatenate([np.arange(1001), [65535, 65536]]), np.arange(65) * 1024,
            np.array([0, 65535, 65536])] + sweep_rows()
    return tables_of(rows, [0, 3, 17, 0] + [5 + 2 * i for i in range(len(rows) - 4)])


def escape_symbol(raw, row, tables):
    """the symbol whose escape value on `row` is raw"""
    _, sizes, offsets = tables
    v0 = -(raw + 1) // 2 if raw & 1 else int(sizes[row]) - 2 + raw // 2
    return v0 + int(offsets[row])


def edge_specials(tables):
    """(sym, idx) every edge stream holds: per row v0 in {-1, 0, max_value - 1, max_value} and an escape of every
    raw value of ESCAPE_RAWS; sym - offset = INT32_MAX and INT32_MIN on the offset-0 rows.  The first nine are the nine
    nibble counts on row A, so that a stream of 64 symbols already holds them all."""
    _, sizes, offsets = tables
    sym, idx = [], []
    first = [0, 1, 16, 256, 16 ** 3, 16 ** 4, 16 ** 5, 16 ** 6, 16 ** 7]
    for raw in first:
        sym.append(escape_symbol(raw, ROW_A, tables))
        idx.append(ROW_A)
    for r in range(len(sizes)):
        maxv, off = int(sizes[r]) - 2, int(offsets[r])
        for v0 in (-1, 0, maxv - 1, maxv):
            sym.append(v0 + off)
            idx.append(r)
        for raw in ESCAPE_RAWS:
            sym.append(escape_symbol(raw, r, tables))
            idx.append(r)
        if off == 0:
            sym += [2 ** 31 - 1, -2 ** 31]
            idx += [r, r]
    return np.asarray(sym, dtype=np.int64).astype(np.int32), np.asarray(idx, dtype=np.uint8)


def edge_case(rng, n, tables, escapes=0.02):
    """n symbols on the edge tables: regular bins of every row, a few escapes, and the specials at shuffled places (as
    many as fit: all of them from n = 4099 on)"""
    _, sizes, offsets = tables
    idx = rng.integers(0, len(sizes), n).astype(np.uint8)
    maxv = sizes[idx].astype(np.int64) - 2
    sym = (rng.integers(0, 1 << 30, n) % np.maximum(maxv, 1)) + offsets[idx]
    k = rng.random(n) < escapes
    sym[k] = rng.integers(-70000, 70000, int(k.sum()))
    s_sym, s_idx = edge_specials(tables)
    m = min(n, s_sym.shape[0])
    at = np.sort(rng.choice(n, m, replace=False)) if n else np.zeros(0, dtype=np.int64)
    sym[at], idx[at] = s_sym[:m], s_idx[:m]
    return sym.astype(np.int32), idx


def plain_case(rng, n, tables, idx_run=0):
    """(sym, idx): regular bins of every row, 2 % escapes, two 8-nibble escapes; idx_run: rows by position and idx None"""
    _, sizes, offsets = tables
    idx = np.arange(n) // idx_run if idx_run else rng.integers(0, len(sizes), n)
    maxv = sizes[idx].astype(np.int64) - 2
    sym = (rng.integers(0, 1 << 30, n) % np.maximum(maxv, 1)) + offsets[idx]
    k = rng.random(n) < 0.02
    sym[k] = rng.integers(-70000, 70000, int(k.sum()))
    if n > 2:
        sym[rng.integers(0, n, 2)] = [2 ** 31 - 1000, -2 ** 31 + 1000]
    return sym.astype(np.int32), None if idx_run else idx.astype(np.uint8)


def nibble_counts(sym, idx, tables, idx_run=1):
    """the set of escape nibble counts a stream holds"""
    sym = np.asarray(sym).reshape(-1)
    _, _, _, nb, esc = lookup(sym, _rows(idx, sym.shape[0], idx_run), tables)
    return set(int(v) for v in nb[esc])
