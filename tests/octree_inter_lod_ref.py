"""The reference of a LEVEL OF DETAIL of octree blob version 4 (include/pcc.h has the rule): the plan of a cut — which
prefix of the blob holds the levels above it — and a decoder of that prefix against the reference's CELLS at the same
lod, in plain Python / numpy over octree_inter_ref.  Its own check (test_octree_inter_lod.py): for every k the plan's
prefix decodes to np.unique(points >> k) in Morton order."""
import struct

import numpy as np

import octree_inter_ref as ref4

LANES, BIAS = ref4.LANES, ref4.BIAS


def morton_cells(cells, k):
    """distinct cells int [m,3] at lod k in the order of their corners' Morton keys (bias 32768)"""
    c = np.unique(np.asarray(cells, np.int64), axis=0)
    return c[np.argsort(ref4.morton((c << k) + BIAS), kind="stable")]


def cells_of(points, k):
    """np.unique(points >> k) in Morton order: what every decoder of lod k returns"""
    return morton_cells(np.asarray(points, np.int64) >> k, k)


def plan(blob, k):
    """the plan of lod k of a version-4 blob, or of a prefix that reaches the last needed chunk's length table: dict of
    Lc (cut level), m (cells), n_dec (nodes needed N'), chunks and lanes (needed; of the last chunk), bytes (shortest
    prefix).  k = 0: the whole blob."""
    h = ref4.header(blob)
    depth, level_n, S, nc = h["depth"], h["level_n"], h["S"], h["nc"]
    if k == 0:
        return dict(Lc=depth, m=h["n"], n_dec=sum(level_n), chunks=nc, lanes=LANES, bytes=24 + h["payload"])
    Lc = max(depth - k, 0)
    m = level_n[Lc] if Lc else 1
    n_dec = sum(level_n[:Lc])
    if n_dec == 0:
        return dict(Lc=Lc, m=m, n_dec=0, chunks=0, lanes=0, bytes=h["off_payload"])
    table = struct.unpack_from("<%dI" % nc, blob, h["off_table"])
    lanes = -(-n_dec // S)
    cs, ls = (lanes - 1) // LANES, (lanes - 1) % LANES
    at = h["off_payload"] + 2 * sum(table[:cs])
    lens = struct.unpack_from("<%dH" % (ls + 1), blob, at + 4 * LANES)
    return dict(Lc=Lc, m=m, n_dec=n_dec, chunks=cs + 1, lanes=ls + 1, bytes=at + 2 * (3 * LANES + sum(lens)))


def decode_lod(prefix, ref_cells, k, bias=BIAS):
    """a prefix of a version-4 blob that holds lod k (k >= 1), the reference's cells at lod k (int [r,3]; the union of a
    window's) -> int64 [m,3] cells of the frame in Morton order.  Nothing of the reference but its cells is used and
    nothing behind the prefix is read; ValueError where the stream does not add up."""
    h, pl = ref4.header(prefix), plan(prefix, k)
    if len(prefix) < pl["bytes"]:
        raise ValueError("truncated")
    depth, S, nc, level_n = h["depth"], h["S"], h["nc"], h["level_n"]
    org = np.array(h["origin"], np.int64) + bias
    if pl["Lc"] == 0:
        return ((org - bias) >> k).reshape(1, 3)
    ref = ref4.Reference(np.asarray(ref_cells, np.int64) << k, bias)      # a cell is searched as its corner
    n_nodes = sum(level_n)
    p0 = list(struct.unpack_from("<%dH" % ref4.CTX4, prefix, h["off_p0"]))
    table = struct.unpack_from("<%dI" % nc, prefix, h["off_table"])
    words = struct.unpack_from("<%dH" % ((pl["bytes"] - h["off_payload"]) // 2), prefix, h["off_payload"])
    lanes, base = [], 0
    for c in range(pl["chunks"]):                     # per lane: state, next word, end of its run, model
        at = base + 3 * LANES
        for l in range(LANES if c + 1 < pl["chunks"] else pl["lanes"]):
            ln = words[base + 2 * LANES + l]
            lanes.append([words[base + 2 * l] | (words[base + 2 * l + 1] << 16), at, at + ln, None])
            at += ln
        if at > len(words) or (c + 1 < pl["chunks"] and at != base + table[c]):
            raise ValueError("chunk length")
        base += table[c]
    start_last = n_nodes - level_n[-1]                # the level classes are the whole tree's
    start_prev = start_last - level_n[-2] if depth >= 2 else 0
    cells, node = np.zeros((1, 3), np.int64), 0
    for L in range(pl["Lc"]):
        if cells.shape[0] != level_n[L]:
            raise ValueError("level size")
        rb = ref.byte(cells, depth - L - 1, org)      # child cubes of side 2^(depth-L-1) >= 2^k: unions of whole cells
        children = []
        for j in range(level_n[L]):
            i = node + j
            lane = lanes[i // S]
            if lane[3] is None:
                lane[3] = list(p0)
            model = lane[3]
            cls = 0 if i >= start_last else (1 if i >= start_prev else 2)
            ones = byte = 0
            for b in range(8):
                if b == 7 and ones == 0:
                    bit = 1
                else:
                    ctx = 108 * ref4._r(rb[j], b) + cls * 36 + b * (b + 1) // 2 + ones
                    p1, x = model[ctx], lane[0]
                    cum = x & 4095
                    bit = 1 if cum >= 4096 - p1 else 0
                    start, freq = (4096 - p1, p1) if bit else (0, 4096 - p1)
                    x = freq * (x >> 12) + cum - start
                    model[ctx] = ref4._adapt(p1, bit)
                    if x < (1 << 16):
                        if lane[1] >= lane[2]:
                            raise ValueError("out of words")
                        x = (x << 16) | words[lane[1]]
                        lane[1] += 1
                    lane[0] = x
                ones += bit
                byte |= bit << b
            cx, cy, cz = cells[j].tolist()
            children += [(2 * cx + ((b >> 2) & 1), 2 * cy + ((b >> 1) & 1), 2 * cz + (b & 1)) for b in range(8) if (byte >> b) & 1]
        node += level_n[L]
        cells = np.array(children, np.int64).reshape(-1, 3)
    whole = pl["n_dec"] // S                           # lanes whose run lies above the cut: every word consumed
    if cells.shape[0] != pl["m"] or any(l[1] != l[2] for l in lanes[:whole]):
        raise ValueError("cell count or words left")
    return ((cells << k) + org - bias) >> k
