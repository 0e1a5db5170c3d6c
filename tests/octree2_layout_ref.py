"""Octree blob version 2 (csrc/octree2_blob.h has the format and the rule of its levels of detail) under ANY layout the
format allows, in plain Python / numpy: a writer that takes S (nodes per lane), the initial table and the occupancy
bytes as given, a reader of the cut tree at every level of detail, and the plan of a level of detail restated from
the bytes.  The coder is octree_inter_ref.encode_payload with the empty context split (its payload is version 2's).
The project's encoders write one layout per node count; the decoder kernels of csrc/octree2.hip read the format."""
import struct

import numpy as np

import octree_inter_ref as ref4

LANES, CTX, SMAX = 64, 108, 512
HEADER = 24
BIAS = 32768
MAX_LOD = 15
DEC_LDS_WORDS = 24576      # kDecLdsWords of csrc/octree2.hip: a longer chunk is read from the stream where it lies


# ------------------------------------------------------------------ writers
def slow_lane(steps):
    """a lane's decisions at ONE WORD EACH, and still a stream every decoder of the format reads without complaint: the
    state starts below 2^12 (no parser looks at a state), there a decision's outcome is `word >= 4096 - p1` and the
    state it leaves is word - start: 0 for the word 0 (a zero) or 4096 - p1 (a one), so the refill that follows puts
    the next such word in its place.  No rANS encoder writes this: its states never leave [2^16, 2^32)."""
    if not steps:
        return 1 << 16, []
    words = [4096 - p1 if bit else 0 for p1, bit in steps]
    return words[0], words[1:] + [0]      # the refill behind the last decision takes a word too


def _assemble(depth, n, origin, level_n, S, nc, p0, chunks):
    body = b"".join(struct.pack("<I", v) for v in level_n) + struct.pack("<II", S, nc)
    body += struct.pack("<%dH" % CTX, *p0) + b"".join(struct.pack("<I", len(ch)) for ch in chunks)
    body += b"".join(struct.pack("<%dH" % len(ch), *ch) for ch in chunks)
    head = bytes([ord("O"), 2, depth, 0]) + struct.pack("<I", n) + struct.pack("<3i", *[int(v) for v in origin])
    return head + struct.pack("<I", len(body)) + body


def encode_bytes(levels, n, origin, S, level_n=None, p0=None, lane=ref4.rans_lane):
    """the blob of the occupancy bytes AS GIVEN (levels: a list of lists, or with level_n one flat list) under the
    announced level sizes and point count; whether the child counts add up is not the coder's business.  origin: the
    header's (unbiased).  S=None: the encoder's layout."""
    flat = [int(b) for lv in levels for b in lv] if level_n is None else [int(b) for b in levels]
    level_n = [len(lv) for lv in levels] if level_n is None else [int(v) for v in level_n]
    if sum(level_n) != len(flat) or not flat:
        raise ValueError("the level sizes announce %d nodes, %d bytes are given" % (sum(level_n), len(flat)))
    at = np.cumsum([0] + level_n)
    split = [flat[at[L]:at[L + 1]] for L in range(len(level_n))]
    S, nc, p0, chunks = ref4.encode_payload(split, [0] * len(flat), CTX, SMAX, S, p0, lane)
    return _assemble(len(level_n), n, origin, level_n, S, nc, p0, chunks)


def encode(points, S=None, p0=None, lane=ref4.rans_lane):
    """blob version 2 of `points` (int [n, 3], duplicates allowed).  S=None: the encoder's layout (the smallest S for
    the chunk count under 512); else any multiple of 4 in 4 .. 512, minimal or not.  p0: the initial table."""
    if np.asarray(points).reshape(-1, 3).shape[0] == 0:
        return bytes([ord("O"), 2, 0, 0]) + bytes(20)
    levels, _, depth, org, n = ref4.build_tree(points, BIAS)
    return encode_bytes(levels, n, [int(v) - BIAS for v in org], S, None, p0, lane)


# ------------------------------------------------------------------ the header, a chunk, the plan of a level of detail
def header(blob):
    """the fields of a version-2 header as a dict (offsets of p0, chunk table and payload; the chunk table as far as
    the bytes hold it)"""
    if len(blob) < HEADER or blob[0] != ord("O") or blob[1] != 2:
        raise ValueError("not a version-2 blob")
    depth = blob[2]
    n, ox, oy, oz, payload = struct.unpack_from("<I3iI", blob, 4)
    h = dict(depth=depth, n=n, origin=(ox, oy, oz), payload=payload)
    if n == 0:
        return h
    if not 1 <= depth <= 16 or len(blob) < HEADER + 4 * depth + 8 + 2 * CTX:
        raise ValueError("truncated header")
    level_n = list(struct.unpack_from("<%dI" % depth, blob, HEADER))
    S, nc = struct.unpack_from("<II", blob, HEADER + 4 * depth)
    off_p0 = HEADER + 4 * depth + 8
    off_table = off_p0 + 2 * CTX
    if len(blob) < off_table + 4 * nc:
        raise ValueError("truncated inside the chunk table")
    h.update(level_n=level_n, n_nodes=sum(level_n), S=S, nc=nc, off_p0=off_p0, off_table=off_table,
             off_payload=off_table + 4 * nc, table=list(struct.unpack_from("<%dI" % nc, blob, off_table)))
    return h


def chunk(blob, c):
    """(byte offset of chunk c, its 64 lane lengths)"""
    h = header(blob)
    at = h["off_payload"] + 2 * sum(h["table"][:c])
    if len(blob) < at + 2 * 3 * LANES:
        raise ValueError("truncated in front of the length table of chunk %d" % c)
    return at, np.array(struct.unpack_from("<64H", blob, at + 2 * 2 * LANES), np.int64)


def plan(blob, lod):
    """the rule of octree2_blob.h read off the bytes of a well-formed blob (or of a prefix that reaches the last
    needed chunk's length table): dict(Lc, cells, nodes = N', lanes, c_star, l_star, bytes); lanes = 0 and
    c_star = l_star = None where no node is decoded"""
    h = header(blob)
    out = dict(Lc=0, cells=0, nodes=0, lanes=0, c_star=None, l_star=None, bytes=HEADER)
    if h["n"] == 0:
        return out
    d, S = h["depth"], h["S"]
    if lod == 0:
        lanes = -(-h["n_nodes"] // S)
        out.update(Lc=d, cells=h["n"], nodes=h["n_nodes"], lanes=lanes, c_star=h["nc"] - 1, l_star=(lanes - 1) % LANES,
                   bytes=HEADER + h["payload"])
        return out
    Lc = max(d - lod, 0)
    need = sum(h["level_n"][:Lc])
    out.update(Lc=Lc, cells=h["level_n"][Lc] if Lc > 0 else 1, nodes=need, bytes=h["off_payload"])
    if need == 0:
        return out
    lanes = -(-need // S)
    c, l = (lanes - 1) // LANES, (lanes - 1) % LANES
    at, lens = chunk(blob, c)
    out.update(lanes=lanes, c_star=c, l_star=l, bytes=at + 2 * (3 * LANES + int(lens[:l + 1].sum())))
    return out


# ------------------------------------------------------------------ the reader
def _adapt(p, bit):
    return p + ((4096 - p) >> 4) if bit else p - (p >> 4)


def decode_bytes(blob, lod=0):
    """(header, plan, the occupancy bytes of the first N' nodes) of a blob or of a prefix that holds plan["bytes"];
    ValueError where k_o2_dec sets status bit 1 (a lane out of words, words left over, a chunk whose lengths and table
    entry disagree) and where the parser refuses (a prefix too short, chunks that do not fill the payload)"""
    h = header(blob)
    pl = plan(blob, lod)
    if len(blob) < pl["bytes"]:
        raise ValueError("truncated: level of detail %d needs %d bytes, %d are here" % (lod, pl["bytes"], len(blob)))
    if h["n"] == 0 or pl["nodes"] == 0:
        return h, pl, []
    d, S, level_n, n_nodes, table = h["depth"], h["S"], h["level_n"], h["n_nodes"], h["table"]
    if S % 4 or not 4 <= S <= SMAX or not LANES * S * (h["nc"] - 1) < n_nodes <= LANES * S * h["nc"]:
        raise ValueError("%d nodes in %d chunks of 64 x %d" % (n_nodes, h["nc"], S))
    if any(cw < 3 * LANES for cw in table) or h["off_payload"] + 2 * sum(table) != HEADER + h["payload"]:
        raise ValueError("the chunks do not fill the payload")
    need, cut = pl["nodes"], pl["nodes"] < n_nodes
    start_last = n_nodes - level_n[-1]
    start_prev = start_last - level_n[-2] if d >= 2 else 0
    p0 = struct.unpack_from("<%dH" % CTX, blob, h["off_p0"])
    occ = []
    for c in range(pl["c_star"] + 1):
        at, lens = chunk(blob, c)
        last = c == pl["c_star"]
        here = pl["l_star"] + 1 if last and cut else LANES
        have = 3 * LANES + int(lens[:here].sum())
        if not (last and cut) and have != table[c]:
            raise ValueError("status 1: the lengths of chunk %d say %d words, its table entry %d" % (c, have, table[c]))
        if last and cut and have > table[c]:
            raise ValueError("the runs of chunk %d take %d words of its %d" % (c, have, table[c]))
        words = struct.unpack_from("<%dH" % have, blob, at)
        pos = 3 * LANES
        for l in range(LANES):
            node0 = (LANES * c + l) * S
            end = pos + int(lens[l]) if l < here else pos
            if l < here and node0 < need:
                x = words[2 * l] | (words[2 * l + 1] << 16)
                model = list(p0)
                for i in range(node0, min(node0 + S, need)):
                    cls = 0 if i >= start_last else (1 if i >= start_prev else 2)
                    ones = byte = 0
                    for j in range(8):
                        if j == 7 and ones == 0:
                            bit = 1
                        else:
                            ctx = cls * 36 + j * (j + 1) // 2 + ones
                            p1, cum = model[ctx], x & 4095
                            bit = 1 if cum >= 4096 - p1 else 0
                            start, freq = (4096 - p1, p1) if bit else (0, 4096 - p1)
                            x = (freq * (x >> 12) + cum - start) & 0xFFFFFFFF
                            model[ctx] = _adapt(p1, bit)
                            if x < (1 << 16):
                                if pos >= end:
                                    raise ValueError("status 1: lane %d of chunk %d is out of words" % (l, c))
                                x = (x << 16) | words[pos]
                                pos += 1
                        ones += bit
                        byte |= bit << j
                    occ.append(byte)
            # every word consumed, but for the lanes of a cut tree whose runs go on (or lie) behind node N' - 1
            if l < here and pos != end and not (cut and need - node0 < S):
                raise ValueError("status 1: lane %d of chunk %d leaves %d words" % (l, c, end - pos))
            pos = end
    assert len(occ) == need
    return h, pl, occ


def decode(blob, lod=0):
    """a blob, or a prefix that holds the plan's bytes -> int64 [cells, 3]: the distinct cells p >> lod of the frame's
    points in Morton order (lod 0: the points).  ValueError as decode_bytes, and where k_o2_link sets status bit 8: a
    level above the cut that does not begin where the header says, children that are not N' + cells - 1 in all"""
    h, pl, occ = decode_bytes(blob, lod)
    if h["n"] == 0:
        return np.zeros((0, 3), np.int64)
    org = np.array(h["origin"], np.int64)
    if pl["nodes"] == 0:
        return (org >> lod).reshape(1, 3)
    Lc, level_n = pl["Lc"], h["level_n"]
    pc = np.array([bin(b).count("1") for b in occ], np.int64)
    first = 1 + np.concatenate([[0], np.cumsum(pc)[:-1]])      # the first child of node i
    off = np.cumsum([0] + level_n[:Lc])
    for L in range(Lc):
        if first[off[L]] != off[L + 1]:
            raise ValueError("status 8: level %d begins at node %d, the header says %d" % (L + 1, first[off[L]], off[L + 1]))
    if int(pc.sum()) != pl["nodes"] + pl["cells"] - 1:
        raise ValueError("status 8: %d children, the header announces %d" % (int(pc.sum()), pl["nodes"] + pl["cells"] - 1))
    cells = np.zeros((1, 3), np.int64)
    octant = np.array([[(j >> 2) & 1, (j >> 1) & 1, j & 1] for j in range(8)], np.int64)
    for L in range(Lc):
        b = np.array(occ[off[L]:off[L + 1]], np.int64)
        has = ((b[:, None] >> np.arange(8)) & 1).astype(bool)      # [nodes, 8]
        cells = (2 * cells[:, None, :] + octant[None, :, :])[has]
    return cells + (org >> lod)


def status(blob, lod=0):
    """0, or the status bit the decoder kernels set for this blob (1 or 8), read off decode's refusal"""
    try:
        decode(blob, lod)
    except ValueError as e:
        msg = str(e)
        if msg.startswith("status "):
            return int(msg.split()[1].rstrip(":"))
        raise
    return 0
