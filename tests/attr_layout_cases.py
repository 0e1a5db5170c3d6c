"""What tests/test_attr_layouts.py (host) and tests/test_gpu_attr_decoder_edges.py (GPU) share: the layouts, fills and
initial tables that the parsers of csrc/attr_blob.h accept and GeometryCodec.compress never writes, the frames they are
tried on, and the room k_a_dec has for a chunk's words in LDS.  Blobs come from the numpy restatements (attr_ref,
attr2_ref, attr_nl_ref, attr_cross_ref) with layout= and p0=.

A layout is (S, n_chunks): S points per lane run, 64 lanes per chunk.  The parsers take it for n > 0 points of c
channels when S >= 1, S c <= 512, 1 <= n_chunks <= n and 64 S (n_chunks - 1) < n <= 64 S n_chunks
(attr_ref.check_layout); the encoder only writes attr_ref.layout(n, c)."""
import struct

import numpy as np

import attr2_ref
from attr_ref import HEAD, LANES, MAX_VALUES, contexts, layout
from conftest import random_cloud

# name -> (n, c, bpv): the two frames of the sweeps
FRAMES = {"1000x3 uint8": (1000, 3, 1), "700x2 uint16": (700, 2, 2)}


def room(bpv, c):
    """the words of a chunk that k_a_dec keeps in LDS beside the models of a call whose widest frame has (bpv, c)
    (a_dec_lds in csrc/attr.hip): 128 KB less nctx + 1 model rows of 64 uint16, in 16-bit words.  A chunk with more
    words than that is read where it lies in HBM.  nctx = 80 c bpv, so the room is 65472 - 5120 c bpv"""
    return (131072 - 128 * (contexts(bpv, c) + 1)) // 2


# room(bpv, c) written out, so that a change of the formula on either side shows
ROOMS = {(1, 1): 60352, (1, 2): 55232, (1, 3): 50112, (1, 4): 44992, (2, 1): 55232, (2, 2): 44992, (2, 3): 34752, (2, 4): 24512}


def values(n, c, bpv, seed):
    """int64 [n, c]: a slow ramp per channel with noise, so that every bucket of the context is used, and runs of both
    extremes"""
    rng = np.random.default_rng(seed)
    hi = (1 << (8 * bpv)) - 1
    ramp = (np.arange(n)[:, None] * (np.arange(c) + 3) * (hi // 97 + 1) // 16) % (hi + 1)
    v = (ramp + rng.integers(-40, 41, (n, c)) * rng.integers(0, 2, (n, c))) % (hi + 1)
    v[::17] = 0
    v[1::17] = hi
    v[5::23] = rng.integers(0, hi + 1, v[5::23].shape)
    return v.astype(np.int64)


def points(n, seed):
    """int32 [n, 3] distinct, some negative, in no order"""
    return random_cloud(np.random.default_rng(seed), n, extent=max(8, int(round((4 * n) ** (1 / 3))) + 2), lo=-9)[:, 1:].astype(np.int32)


def morton(pts, vals):
    """distinct points and their values, both in Morton order"""
    o = np.argsort(attr2_ref.keys_of(pts))
    return np.asarray(pts)[o], np.asarray(vals)[o]


def sample(pts, vals, k):
    """points / values in Morton order -> the cells points >> k in Morton order and, per cell, the value of its
    Morton-first point"""
    _, idx = np.unique(attr2_ref.keys_of(pts >> k, 32768 >> k), return_index=True)
    return pts[idx] >> k, vals[idx]


def sweep_layouts(n, c):
    """the encoder's own; one point per lane; three; (8, 2) where n lies in its span; the longest run S c <= 512 allows.
    The chunk count is what the parser's conditions force for that S"""
    out = [layout(n, c)]
    for S in (1, 3, 8, MAX_VALUES // c):
        nc = -(-n // (LANES * S))
        if (S, nc) not in out and (S != 8 or nc == 2):
            out.append((S, nc))
    return out


# (what, n, c, bpv, (S, n_chunks)): how full the last chunk is, and the longest runs
FILLS = [
    ("n = 64 S nc", 960, 3, 1, (3, 5)),
    ("n = 64 S nc", 1024, 2, 2, (8, 2)),
    ("n = 64 S nc", 640, 2, 2, (1, 10)),
    ("n = 64 S (nc - 1) + 1", 961, 3, 1, (3, 6)),           # the last chunk: one point, 63 lanes of len 0 in state 2^16
    ("n = 64 S (nc - 1) + 1", 513, 2, 2, (8, 2)),
    ("n = 64 S (nc - 1) + 1", 641, 3, 1, (1, 11)),
    ("n = 1", 1, 3, 1, (1, 1)),
    ("n = 1", 1, 3, 1, (170, 1)),
    ("n = 1", 1, 2, 2, (256, 1)),
    ("S c = 512", 1000, 1, 1, (512, 1)),                     # two lanes hold the frame
    ("S c = 512", 700, 2, 2, (256, 1)),
    ("S c = 512", 1000, 4, 1, (128, 1)),
    ("S c = 510", 1000, 3, 1, (170, 1)),
]


def chunk_lanes(blob, off_payload, words, k):
    """(final states, lens) of chunk k's 64 lanes, from the blob's own bytes"""
    at = off_payload + 2 * sum(words[:k])
    w = np.frombuffer(blob, "<u2", 192, at).astype(np.int64)
    return w[0:128:2] | (w[1:128:2] << 16), w[128:192]


def head_of(blob):
    """(version, n, S, n_chunks, p0, words per chunk, off_table, off_payload) of an attribute blob of versions 1, 2, 4, 7, 8,
    11, 13 or 14 with points, read from its bytes as the layout comment of csrc/attr_blob.h places them"""
    ver, bpv, c = blob[1], blob[2] & 15, blob[3] & 15
    at = HEAD + (4 if ver in (4, 7, 13, 14) else 0) + (64 if ver in (2, 7, 11, 14) else 0)
    n = struct.unpack_from("<I", blob, 4)[0]
    S, nc = struct.unpack_from("<II", blob, at)
    nctx = contexts(bpv, c)
    p0 = np.frombuffer(blob, "<u2", nctx, at + 8).astype(np.int64)
    off_table = at + 8 + 2 * nctx
    words = list(struct.unpack_from("<%dI" % nc, blob, off_table))
    return ver, n, S, nc, p0, words, off_table, off_table + 4 * nc


def tables(counted, seed):
    """name -> p0: the bounds of what attr_check_p0 takes, alone and side by side; anything between them; and the encoder's
    counted table with its first entry at the lower bound and its second at the upper"""
    nctx = counted.shape[0]
    moved = counted.copy()
    moved[0], moved[1] = 16, 4080
    return {"all 16": np.full(nctx, 16), "all 4080": np.full(nctx, 4080), "16 and 4080 alternating": np.where(np.arange(nctx) % 2, 4080, 16),
            "random": np.random.default_rng(seed).integers(16, 4081, nctx), "counted, one entry at each bound": moved}


def frame(name_or_shape, seed=5):
    """(points [n, 3] in no order, values [n, c] row i belonging to points[i], bpv) of a frame of FRAMES or of (n, c, bpv)"""
    n, c, bpv = FRAMES[name_or_shape] if isinstance(name_or_shape, str) else name_or_shape
    return points(n, seed + n), values(n, c, bpv, seed + 7 * n + c), bpv


def sweep_cases():
    """[(id, points, values, bpv, (S, n_chunks))]: every layout of sweep_layouts for the two frames, then FILLS"""
    out = []
    for name in FRAMES:
        pts, vals, bpv = frame(name)
        out += [("%s (%d, %d)" % ((name,) + lay), pts, vals, bpv, lay) for lay in sweep_layouts(*vals.shape)]
    for what, n, c, bpv, lay in FILLS:
        pts, vals, _ = frame((n, c, bpv))
        out.append(("%s: %dx%d bpv %d (%d, %d)" % ((what, n, c, bpv) + lay), pts, vals, bpv, lay))
    return out


def table_cases():
    """[(id, points, values, bpv, p0)]: every table of tables() for the two frames, under the encoder's layout"""
    import attr_ref
    out = []
    for name in FRAMES:
        pts, vals, bpv = frame(name)
        counted = head_of(attr_ref.encode(vals, bpv))[4]
        out += [("%s p0 %s" % (name, what), pts, vals, bpv, p0) for what, p0 in tables(counted, vals.shape[0]).items()]
    return out


# constructed bad streams: what damage() does to one chunk of a sound blob.  None of them changes what the parsers check
DAMAGE = ("move a word of len 0 -> 1", "move a word of len 31 -> 32", "move a word of len 62 -> 63", "table entry + 1", "table entry - 1",
          "state of lane 63", "len 63 into len 0")


def damage(blob, how, k=0):
    """a copy of a whole blob (versions 1, 2 and their kin) with one of DAMAGE done to chunk k, whose 64 lanes all hold
    points.  The length table still sums to the chunk's words.  "table entry" is done to the last chunk instead: its
    entry says one word more (a word is appended to the blob) or less (the last word is dropped) and payload_len
    follows, so that every sum a parser forms still holds and only 192 + the lens of that chunk disagree with its
    entry"""
    _, _, _, nc, _, words, off_table, off_payload = head_of(blob)
    b = bytearray(blob)
    at = off_payload + 2 * sum(words[:k])
    get = lambda i: struct.unpack_from("<H", b, at + 2 * i)[0]
    put = lambda i, v: struct.pack_into("<H", b, at + 2 * i, v)
    if how.startswith("move a word of len"):
        j = int(how.split()[5])
        assert get(128 + j) >= 1 and get(129 + j) < 65535
        put(128 + j, get(128 + j) - 1)
        put(129 + j, get(129 + j) + 1)
    elif how.startswith("table entry"):
        d = 1 if how.endswith("+ 1") else -1
        struct.pack_into("<I", b, off_table + 4 * (nc - 1), words[-1] + d)
        struct.pack_into("<I", b, 8, struct.unpack_from("<I", b, 8)[0] + 2 * d)
        b = b + b"\x34\x12" if d > 0 else b[:-2]
    elif how == "state of lane 63":
        put(126, get(126) ^ 0x0101)
    elif how == "len 63 into len 0":
        assert get(128 + 63) >= 1 and get(128) + get(128 + 63) < 65536
        put(128, get(128) + get(128 + 63))
        put(128 + 63, 0)
    else:
        raise ValueError(how)
    return bytes(b)
