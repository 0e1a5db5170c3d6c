"""The reference of octree blob version 4 (a predicted frame; include/pcc.h has the rule): an encoder and a decoder in
plain Python / numpy, written from the rule, in the style of test_octree2.py's py_octree2_encode.  Its own check
(test_octree_inter.py): the decoder inverts the encoder, and with the context split taken out (every r forced to 0,
108 entries of p0) the payload is py_octree2_encode's."""
import struct

import numpy as np

LANES, CTX2, CTX4, SMAX4 = 64, 108, 324, 256
BIAS = 32768


# ------------------------------------------------------------------ the tree, as version 2 builds it
def build_tree(points, bias=BIAS):
    """distinct points int [n,3] -> (occupancy bytes per level, cells per level int64 [nodes_L, 3] relative to the root
    cube, depth, origin of the root cube in BIASED coordinates, n); nodes of a level in Morton order, x the top bit"""
    pts = np.unique(np.asarray(points, dtype=np.int64) + bias, axis=0)
    depth = 1
    while not np.all((pts >> depth) == (pts[0] >> depth)):
        depth += 1
    org = (pts[0] >> depth) << depth
    rel = pts - org
    levels, cells = [], []
    for L in range(depth):
        sh = depth - L
        node = rel >> sh
        octant = (((rel[:, 0] >> (sh - 1)) & 1) << 2) | (((rel[:, 1] >> (sh - 1)) & 1) << 1) | ((rel[:, 2] >> (sh - 1)) & 1)
        key = morton(node)
        order = np.argsort(key, kind="stable")
        key, octant, node = key[order], octant[order], node[order]
        first = np.concatenate([[True], key[1:] != key[:-1]])
        idx = np.cumsum(first) - 1
        occ = np.zeros(int(idx[-1]) + 1, np.int64)
        np.bitwise_or.at(occ, idx, 1 << octant)
        levels.append(occ.tolist())
        cells.append(node[first])
    return levels, cells, depth, org, pts.shape[0]


def morton(c):
    c = np.asarray(c, dtype=np.int64)
    key = np.zeros(c.shape[0], np.int64)
    for b in range(16, -1, -1):
        key = (key << 3) | (((c[:, 0] >> b) & 1) << 2) | (((c[:, 1] >> b) & 1) << 1) | ((c[:, 2] >> b) & 1)
    return key


# ------------------------------------------------------------------ the reference byte
def _pack(c):
    """rows of small signed integers -> one int64 each (equal rows, equal numbers)"""
    c = np.asarray(c, dtype=np.int64) + (1 << 18)
    return (c[:, 0] << 40) | (c[:, 1] << 20) | c[:, 2]


class Reference:
    """R: distinct lattice points.  byte(cells, s, org): for nodes whose CHILD cubes have side 2^s and lie at
    org + child_cell * 2^s (biased coordinates), bit j = R has a point inside child j's cube"""

    def __init__(self, points, bias=BIAS):
        self.pts = np.unique(np.asarray(points, dtype=np.int64), axis=0)
        self.biased = self.pts + bias
        self.n = self.pts.shape[0]
        self.sum = int(sum(((int(x) & 0xFFFF) << 32) | ((int(y) & 0xFFFF) << 16) | (int(z) & 0xFFFF)
                           for x, y, z in self.pts.tolist()) % (1 << 64))
        self._sets = {}

    def byte(self, cells, s, org):
        k = (s, tuple(int(v) for v in org))
        if k not in self._sets:      # the cells of side 2^s, in the frame's grid, that hold a point of R
            self._sets[k] = np.unique(_pack((self.biased - np.asarray(org, np.int64)) >> s))
        have = self._sets[k]
        cells = np.asarray(cells, dtype=np.int64)
        out = np.zeros(cells.shape[0], np.int64)
        for j in range(8):
            child = 2 * cells + np.array([(j >> 2) & 1, (j >> 1) & 1, j & 1])
            q = _pack(child)
            at = np.searchsorted(have, q)
            hit = (at < have.shape[0]) & (have[np.minimum(at, have.shape[0] - 1)] == q)
            out |= hit.astype(np.int64) << j
        return out.tolist()


def reference_bytes(cells, depth, org, ref):
    """the reference byte of every node, breadth-first"""
    rb = []
    for L in range(depth):
        rb += ref.byte(cells[L], depth - L - 1, org)
    return rb


# ------------------------------------------------------------------ the coder
def _p0(c0, c1):
    return min(4080, max(16, (4096 * (2 * c1 + 1)) // (2 * (c0 + c1 + 1))))


def _adapt(p, bit):
    return p + ((4096 - p) >> 4) if bit else p - (p >> 4)


def _r(rbyte, j):
    return 0 if rbyte == 0 else 1 + ((rbyte >> j) & 1)


def _layout(n_nodes, smax):
    nc = max(1, -(-n_nodes // (LANES * smax)))
    S = max(4, -(-(-(-n_nodes // (LANES * nc))) // 4) * 4)
    return S, nc


def _forced_layout(n_nodes, S):
    """a layout the format allows and no encoder of the project chooses: any multiple of 4 in 4 .. 512 as S, minimal
    or not; the chunk count is what S makes it"""
    if S != int(S) or S % 4 or not 4 <= S <= 512:
        raise ValueError("S must be a multiple of 4 in 4 .. 512")
    return int(S), max(1, -(-n_nodes // (LANES * int(S))))


def rans_lane(steps):
    """(final state, words in the order a decoder consumes them) of a lane's decisions [(probability of a one, bit)]"""
    x, words = 1 << 16, []
    for p1, bit in reversed(steps):
        freq, start = (p1, 4096 - p1) if bit else (4096 - p1, 0)
        if x >= freq << 20:
            words.append(x & 0xFFFF)
            x >>= 16
        x = ((x // freq) << 12) + x % freq + start
    return x, words[::-1]


def encode_payload(levels, rb, n_ctx, smax, S=None, p0=None, lane=rans_lane):
    """(S, nc, p0, chunks): the lanes' rANS streams of the occupancy bytes under contexts r * 108 + version 2's.
    S=None: the encoder's layout under the bound smax; else S nodes per lane as given (lanes behind the last node
    carry the initial state and no words).  p0: the initial table as given instead of the counted one; lane: another
    writer of a lane's decisions (octree2_layout_ref has one)"""
    occ = [b for lv in levels for b in lv]
    depth, n_nodes = len(levels), len(occ)
    S, nc = _layout(n_nodes, smax) if S is None else _forced_layout(n_nodes, S)
    start_last = n_nodes - len(levels[-1])
    start_prev = start_last - len(levels[-2]) if depth >= 2 else 0

    def decisions(i):
        cls = 0 if i >= start_last else (1 if i >= start_prev else 2)
        ones = 0
        for j in range(8):
            bit = (occ[i] >> j) & 1
            if j == 7 and ones == 0:
                return
            yield 108 * _r(rb[i], j) + cls * 36 + j * (j + 1) // 2 + ones, bit
            ones += bit

    c0, c1 = [0] * n_ctx, [0] * n_ctx
    for i in range(n_nodes):
        for ctx, bit in decisions(i):
            (c1 if bit else c0)[ctx] += 1
    p0 = [_p0(c0[k], c1[k]) for k in range(n_ctx)] if p0 is None else [int(v) for v in p0]
    if len(p0) != n_ctx or not all(16 <= v <= 4080 for v in p0):
        raise ValueError("p0: %d probabilities in 16 .. 4080" % n_ctx)
    chunks = []
    for c in range(nc):
        states, lens, runs = [], [], []
        for l in range(LANES):
            model, steps = list(p0), []
            for s in range(S):
                i = (LANES * c + l) * S + s
                if i >= n_nodes:
                    break
                for ctx, bit in decisions(i):
                    steps.append((model[ctx], bit))
                    model[ctx] = _adapt(model[ctx], bit)
            x, words = lane(steps)
            states += [x & 0xFFFF, x >> 16]
            lens.append(len(words))
            runs += words
        chunks.append(states + lens + runs)
    return S, nc, p0, chunks


def encode(points, reference, bias=BIAS, split=True, smax=SMAX4, S=None):
    """blob version 4 of `points` (int [n,3], duplicates allowed) against the points `reference`.  split=False: the
    empty context split (every r = 0, 108 entries of p0), whose payload is version 2's.  S: a forced layout
    (encode_payload), for blobs a decoder must read and the project's encoder never writes."""
    levels, cells, depth, org, n = build_tree(points, bias)
    ref = reference if isinstance(reference, Reference) else Reference(reference, bias)
    n_nodes = sum(len(lv) for lv in levels)
    rb = reference_bytes(cells, depth, org, ref) if split else [0] * n_nodes
    S, nc, p0, chunks = encode_payload(levels, rb, CTX4 if split else CTX2, smax, S)
    body = b"".join(struct.pack("<I", len(lv)) for lv in levels) + struct.pack("<II", S, nc)
    body += struct.pack("<IQ", ref.n, ref.sum)
    body += struct.pack("<%dH" % len(p0), *p0) + b"".join(struct.pack("<I", len(ch)) for ch in chunks)
    body += b"".join(struct.pack("<%dH" % len(ch), *ch) for ch in chunks)
    head = bytes([ord("O"), 4, depth, 0]) + struct.pack("<I", n) + struct.pack("<3i", *[int(v) - bias for v in org])
    return head + struct.pack("<I", len(body)) + body


def header(blob):
    """the fields of a version-4 header as a dict (offsets of p0, chunk table and payload included)"""
    assert blob[0] == ord("O") and blob[1] == 4
    depth = blob[2]
    n, ox, oy, oz, payload = struct.unpack_from("<I3iI", blob, 4)
    level_n = list(struct.unpack_from("<%dI" % depth, blob, 24))
    at = 24 + 4 * depth
    S, nc, ref_n, ref_sum = struct.unpack_from("<IIIQ", blob, at)
    off_p0 = at + 20
    off_table = off_p0 + 2 * CTX4
    return dict(depth=depth, n=n, origin=(ox, oy, oz), payload=payload, level_n=level_n, S=S, nc=nc, ref_n=ref_n, ref_sum=ref_sum,
                off_p0=off_p0, off_table=off_table, off_payload=off_table + 4 * nc)


def decode(blob, reference, bias=BIAS):
    """version-4 blob -> int64 [n,3] points in Morton order; ValueError where the reference is another or the stream
    does not add up"""
    h = header(blob)
    ref = reference if isinstance(reference, Reference) else Reference(reference, bias)
    if (ref.n, ref.sum) != (h["ref_n"], h["ref_sum"]):
        raise ValueError("the reference differs")
    depth, S, nc, level_n = h["depth"], h["S"], h["nc"], h["level_n"]
    n_nodes = sum(level_n)
    p0 = list(struct.unpack_from("<%dH" % CTX4, blob, h["off_p0"]))
    table = struct.unpack_from("<%dI" % nc, blob, h["off_table"])
    words = struct.unpack_from("<%dH" % ((len(blob) - h["off_payload"]) // 2), blob, h["off_payload"])
    lanes, base = [], 0
    for c in range(nc):                               # per lane: state, next word, end of its run, model
        at = base + 3 * LANES
        for l in range(LANES):
            ln = words[base + 2 * LANES + l]
            lanes.append([words[base + 2 * l] | (words[base + 2 * l + 1] << 16), at, at + ln, None])
            at += ln
        if at != base + table[c]:
            raise ValueError("chunk length")
        base += table[c]
    start_last = n_nodes - level_n[-1]
    start_prev = start_last - level_n[-2] if depth >= 2 else 0
    org = np.array(h["origin"], np.int64) + bias
    cells, node = np.zeros((1, 3), np.int64), 0
    for L in range(depth):
        if cells.shape[0] != level_n[L]:
            raise ValueError("level size")
        rb = ref.byte(cells, depth - L - 1, org)
        children = []
        for k in range(level_n[L]):
            i = node + k
            lane = lanes[i // S]
            if lane[3] is None:
                lane[3] = list(p0)
            model = lane[3]
            cls = 0 if i >= start_last else (1 if i >= start_prev else 2)
            ones = byte = 0
            for j in range(8):
                if j == 7 and ones == 0:
                    bit = 1
                else:
                    ctx = 108 * _r(rb[k], j) + cls * 36 + j * (j + 1) // 2 + ones
                    p1, x = model[ctx], lane[0]
                    cum = x & 4095
                    bit = 1 if cum >= 4096 - p1 else 0
                    start, freq = (4096 - p1, p1) if bit else (0, 4096 - p1)
                    x = freq * (x >> 12) + cum - start
                    model[ctx] = _adapt(p1, bit)
                    if x < (1 << 16):
                        if lane[1] >= lane[2]:
                            raise ValueError("out of words")
                        x = (x << 16) | words[lane[1]]
                        lane[1] += 1
                    lane[0] = x
                ones += bit
                byte |= bit << j
            cx, cy, cz = cells[k].tolist()
            children += [(2 * cx + ((j >> 2) & 1), 2 * cy + ((j >> 1) & 1), 2 * cz + (j & 1)) for j in range(8) if (byte >> j) & 1]
        node += level_n[L]
        cells = np.array(children, np.int64).reshape(-1, 3)
    if cells.shape[0] != h["n"] or any(l[1] != l[2] for l in lanes):
        raise ValueError("point count or words left")
    return cells + org - bias
