"""Inputs and a second reference for the coordinate-map and pyramid tests (tests/test_map_edges.py,
tests/test_pyramid_edges.py).  Plain numpy; nothing of the package is imported.  The restatements here (Morton key,
hash64, hash_capacity) are held to the oracle and to themselves on the CPU; csrc/map.hip names this file at the two
functions it restates, because the probe-chain inputs are only chains while those stay as they are."""
import functools

import numpy as np

U = np.uint64
LO, HI = -32768, 32767
OFFS = np.array([(k // 9 - 1, (k // 3) % 3 - 1, k % 3 - 1) for k in range(27)], dtype=np.int64)   # k -> (dx, dy, dz)
HASH_EMPTY = (1 << 64) - 1


# ------------------------------------------------------------------ restatements
def _u(a):
    return np.atleast_1d(np.asarray(a)).astype(U)


def _spread3(v):
    x = _u(v) & U(0xFFFF)
    x = (x | (x << U(16))) & U(0x0000FF0000FF)
    x = (x | (x << U(8))) & U(0x00F00F00F00F)
    x = (x | (x << U(4))) & U(0x0C30C30C30C3)
    x = (x | (x << U(2))) & U(0x249249249249)
    return x


def _compact3(x):
    x = _u(x) & U(0x249249249249)
    x = (x | (x >> U(2))) & U(0x0C30C30C30C3)
    x = (x | (x >> U(4))) & U(0x00F00F00F00F)
    x = (x | (x >> U(8))) & U(0x0000FF0000FF)
    x = (x | (x >> U(16))) & U(0xFFFF)
    return x


def morton(b, x, y, z):
    """key = b << 48 | x bits at 3i+2, y at 3i+1, z at 3i, coordinates biased by 32768 (and masked to 16 bits, as the
    kernels' spread does: a caller that wants the range checked checks it)"""
    bias = np.int64(32768)
    return ((_u(b) << U(48)) | (_spread3(np.asarray(x, np.int64) + bias) << U(2)) |
            (_spread3(np.asarray(y, np.int64) + bias) << U(1)) | _spread3(np.asarray(z, np.int64) + bias))


def unmorton(keys):
    k = _u(keys)
    return ((k >> U(48)).astype(np.int64), _compact3(k >> U(2)).astype(np.int64) - 32768,
            _compact3(k >> U(1)).astype(np.int64) - 32768, _compact3(k).astype(np.int64) - 32768)


def coords_keys(c):
    c = np.asarray(c, dtype=np.int64).reshape(-1, 4)
    return morton(c[:, 0], c[:, 1], c[:, 2], c[:, 3])


def sorted_keys(c):
    return np.sort(coords_keys(c))


C1, C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
C1_INV, C2_INV = pow(C1, -1, 1 << 64), pow(C2, -1, 1 << 64)


def hash64(k):
    k = _u(k).copy()
    k ^= k >> U(33)
    k *= U(C1)
    k ^= k >> U(33)
    k *= U(C2)
    k ^= k >> U(33)
    return k


def hash64_inv(h):
    """x ^= x >> 33 is its own inverse (2 * 33 > 64); the odd multipliers are inverted mod 2^64"""
    k = _u(h).copy()
    k ^= k >> U(33)
    k *= U(C2_INV)
    k ^= k >> U(33)
    k *= U(C1_INV)
    k ^= k >> U(33)
    return k


def hash_capacity(n):
    cap = 1024
    while cap < 4 * n:
        cap <<= 1
    return cap


# ------------------------------------------------------------------ references
def map27_ref(keys, stride, unchecked_axis=None):
    """[27, n] rule book of sorted distinct keys.  unchecked_axis = 0 / 1 / 2: the book a kernel would give that
    forgot the range check of x / y / z (the coordinate wraps mod 2^16 onto the opposite face)"""
    keys = _u(keys)
    n = keys.shape[0]
    b, x, y, z = unmorton(keys)
    nbr = np.full((27, n), -1, dtype=np.int32)
    if n == 0:
        return nbr
    for k in range(27):
        if k == 13:
            nbr[k] = np.arange(n, dtype=np.int32)
            continue
        c = [x + OFFS[k, 0] * stride, y + OFFS[k, 1] * stride, z + OFFS[k, 2] * stride]
        ok = np.ones(n, dtype=bool)
        for ax in range(3):
            if ax != unchecked_axis:
                ok &= (c[ax] >= LO) & (c[ax] <= HI)
        q = morton(b, c[0], c[1], c[2])
        at = np.minimum(np.searchsorted(keys, q), n - 1)
        hit = ok & (keys[at] == q)
        nbr[k] = np.where(hit, at, -1).astype(np.int32)
    return nbr


def hit_share(nbr):
    """share of the 26 n non-centre entries of a book that are rows"""
    n = nbr.shape[1]
    return float((np.delete(nbr, 13, axis=0) >= 0).sum()) / (26 * n)


def wrap_entries(keys, stride):
    """per axis, the (offset, row) entries that are -1 and that a missing check of that axis alone would turn into a
    row: [3] arrays of shape [e, 2]"""
    ref = map27_ref(keys, stride)
    out = []
    for ax in range(3):
        bad = map27_ref(keys, stride, unchecked_axis=ax)
        out.append(np.argwhere((ref < 0) & (bad >= 0)))
    return out


def down_ref(keys, cshift):
    """(pkeys [m], nbr8 [8, m], parent_of [n]) of a stride-2 kernel-2 stage over sorted distinct keys"""
    keys = _u(keys)
    s = U(cshift + 3)
    pkeys, parent_of = np.unique((keys >> s) << s, return_inverse=True)
    parent_of = parent_of.reshape(-1)
    nbr8 = np.full((8, pkeys.shape[0]), -1, dtype=np.int32)
    o = ((keys >> U(cshift)) & U(7)).astype(np.int64)
    nbr8[o, parent_of] = np.arange(keys.shape[0], dtype=np.int32)
    return pkeys, nbr8, parent_of.astype(np.int32)


def up_keys(keys, cshift):
    """the 8 generative children of every key, parent-major (already sorted)"""
    return (_u(keys)[:, None] | (np.arange(8, dtype=U) << U(cshift))[None, :]).reshape(-1)


def level_counts_ref(keys, cshift, levels):
    keys = _u(keys)
    counts = [int(np.unique(keys >> U(cshift + 3 * (l + 1))).shape[0]) for l in range(levels)]
    return counts, bool(np.any(keys[1:] == keys[:-1]))


def diff_bits(keys):
    """set of the highest differing bit over neighbouring pairs of distinct sorted keys (the histogram's bins)"""
    x = _u(keys)
    x = x[1:] ^ x[:-1]
    x = x[x != 0]
    top = np.zeros(x.shape[0], dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> U(s)) != 0
        top += np.where(big, s, 0)
        x = np.where(big, x >> U(s), x)
    return set(int(v) for v in np.unique(top))


# ------------------------------------------------------------------ clouds
def lattice_cloud(rng, n, stride, batches=2, box=None, batch_ids=None):
    """[n, 4] (b, x, y, z) int32: n distinct points drawn without replacement from `batches` cubes of together about
    `box` cells (default 3 n) that straddle zero, times `stride`"""
    box = 3 * n if box is None else box
    side = max(1, int(round((box / batches) ** (1.0 / 3.0))))
    while batches * side ** 3 < n:
        side += 1
    lo = -(side // 2)
    assert lo * stride >= LO and (lo + side - 1) * stride <= HI, "the box leaves the coordinate range"
    pick = rng.choice(batches * side ** 3, size=n, replace=False).astype(np.int64)
    b, r = np.divmod(pick, side ** 3)
    if batch_ids is not None:
        b = np.asarray(batch_ids, dtype=np.int64)[b]
    c = np.stack([b, (r // (side * side) + lo) * stride, ((r // side) % side + lo) * stride, (r % side + lo) * stride], 1)
    return c.astype(np.int32)


def pad_keys(rng, head_keys, n, stride, **kw):
    """sorted distinct keys, n in all: head_keys and lattice_cloud rows that are none of them"""
    head = np.unique(_u(head_keys))
    more = sorted_keys(lattice_cloud(rng, n, stride, **kw))
    more = more[~np.isin(more, head)][: n - head.shape[0]]
    keys = np.sort(np.concatenate([head, more]))
    assert keys.shape[0] == n and np.all(keys[1:] > keys[:-1])
    return keys


def wrap_rows(stride):
    """(coords [r, 4], per-axis wrap entries of their book): pairs of rows on opposite faces of the cube, which are
    neighbours mod 2^16 and not neighbours.  With stride s the last lattice point is 32768 - s, and + s wraps it onto
    -32768, a lattice point again."""
    s, h, l = stride, 32768 - stride, LO
    rows = []
    for ax in range(3):                                  # one axis, same batch / different batches
        for bh, bl in ((0, 0), (2, 3)):
            for v, b in ((h, bh), (l, bl)):
                c = [0, -s]
                c.insert(ax, v)
                rows.append([b] + c)
    for ax in range(3):                                  # two axes at once
        for v in (h, l):
            c = [v, v]
            c.insert(ax, 0)
            rows.append([4] + c)
    rows += [[5, h, h, h], [5, l, l, l], [6, h, h, h]]   # the full diagonal; a corner with nothing opposite
    c = np.asarray(rows, dtype=np.int32)
    assert np.unique(c, axis=0).shape[0] == c.shape[0]
    return c, wrap_entries(sorted_keys(c), stride)


def collision_chain(cap, slot, length, rng, stride=1):
    """(chain keys [length], witness keys): valid keys (batch index <= 65534) whose home slot in a table of `cap`
    slots is `slot`, from the inverse of hash64; a witness is the point at + (stride, 0, 0) of a chain key, so that its
    offset 4 = (-1, 0, 0) is the chain key"""
    got = np.zeros(0, dtype=U)
    while got.shape[0] < length:
        j = rng.integers(0, (1 << 64) // cap, size=4 * length, dtype=np.uint64)
        k = hash64_inv(U(slot) + U(cap) * j)
        k = k[(k >> U(48)) <= U(65534)]
        got = np.unique(np.concatenate([got, k]))
    got = rng.permutation(got)[:length]
    assert np.all((hash64(got) & U(cap - 1)) == U(slot)) and np.unique(got).shape[0] == length
    assert not np.any(got == U(HASH_EMPTY))
    b, x, y, z = unmorton(got)
    ok = x + stride <= HI
    return got, morton(b[ok], x[ok] + stride, y[ok], z[ok])


# ------------------------------------------------------------------ parents
_RANK = np.array([np.roll(np.array([0, 5, 2, 7, 4, 1, 6, 3]), r) for r in range(8)])   # octant -> rank, per p % 8
PATTERNS = ("cycle", "cycle7", "eights") + tuple("eights+%d" % o for o in range(1, 8)) + ("singles", "random")


def _sizes(n, pattern, rng):
    if pattern == "singles":
        return np.ones(n, dtype=np.int64)
    if pattern == "random":
        c = rng.integers(1, 9, size=n)
    elif pattern.startswith("eights"):
        o = int(pattern[7:]) if "+" in pattern else 0
        c = np.concatenate([np.ones(o, dtype=np.int64), np.full(n // 8 + 1, 8, dtype=np.int64)])
    else:
        p = 7 if pattern == "cycle7" else 8
        c = np.tile(np.arange(1, p + 1), n // (p * (p + 1) // 2) + 1)
    c = c[: int(np.searchsorted(np.cumsum(c), n)) + 1].astype(np.int64)
    c[-1] -= c.sum() - n
    return c


@functools.lru_cache(maxsize=6)
def parent_runs(n, pattern, cshift, batches=1, seed=0):
    """(keys [n] sorted distinct with the low cshift bits zero, (s8, s512, s2048)): the sizes of successive parents
    follow `pattern`; s_B = parents with children on both sides of a multiple of B rows.  batches > 1 (a tuple of batch
    indexes): the same low 48 bits in every batch, n / len(batches) keys each."""
    rng = np.random.default_rng(seed)
    ids = (0,) if batches == 1 else tuple(batches)
    per = n // len(ids)
    assert per * len(ids) == n
    c = _sizes(per, pattern, rng)
    m = c.shape[0]
    v = np.cumsum(rng.integers(1, 4, size=m)).astype(np.int64)             # parent values: gaps of 1 .. 3
    mask = _RANK[np.arange(m) % 8] < c[:, None]                            # [m, 8]: the octants of parent p
    p, o = np.nonzero(mask)
    low = ((v[p].astype(U) << U(3)) | o.astype(U)) << U(cshift)
    if len(ids) > 1:
        assert int(low.max()) < 1 << 48
    keys = np.concatenate([(U(b) << U(48)) + low for b in ids])
    assert keys.shape[0] == n and np.all(keys[1:] > keys[:-1]) and int(keys.max() >> U(48)) <= 65534
    first = np.concatenate([[0], np.cumsum(c)[:-1]])
    first = np.concatenate([first + i * per for i in range(len(ids))])
    last = first + np.tile(c, len(ids)) - 1
    seams = tuple(int(((first // B) != (last // B)).sum()) for B in (8, 512, 2048))
    keys.setflags(write=False)
    return keys, seams
