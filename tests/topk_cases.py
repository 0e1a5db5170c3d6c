"""Seeded inputs for tests/test_topk_edges.py: the edges of the top-k pruning (csrc/topk.hip), built from the
integer keys the radix select walks rather than from floats, and a numpy restatement of the rule.
No GPU in here.  Every generator is cached; callers must leave what they get unchanged."""
import functools

import numpy as np

SIGN = np.uint32(0x80000000)


def ordered_key(x):
    """the order-preserving integer image of a float32 (topk.hip ordered_key, pcc_oracle.c ordered_key)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & SIGN, ~u, u | SIGN).astype(np.uint32)


def float_from_key(k):
    """inverse of ordered_key: top bit set -> clear it, else complement.  Reinterpreted, never converted: NaN
    payloads survive"""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & SIGN, k & ~SIGN, ~k).astype(np.uint32).view(np.float32)


def offsets_of(counts):
    return [0] + [int(v) for v in np.cumsum(np.asarray(counts, dtype=np.int64))]


def topk_ref(logits, offsets, k):
    """The rule by a route of its own: per frame sort by (key descending, row ascending), take min(k, count),
    rows ascending."""
    keys = ordered_key(logits).astype(np.int64)
    out = []
    for f in range(len(k)):
        lo, hi = int(offsets[f]), int(offsets[f + 1])
        take = min(int(k[f]), hi - lo)
        if take <= 0:
            continue
        rows = np.arange(lo, hi, dtype=np.int64)
        order = np.lexsort((rows, -keys[lo:hi]))          # the last key is the primary one
        out.append(np.sort(rows[order[:take]]))
    return np.concatenate(out).astype(np.uint32) if out else np.empty(0, np.uint32)


def remap_ref(n, rows):
    """position of a row among the kept ones, else -1"""
    want = np.full(n, -1, np.int32)
    want[rows.astype(np.int64)] = np.arange(len(rows), dtype=np.int32)
    return want


def threshold_key(logits, offsets, k, f):
    """key of the k[f]-th largest row of frame f: what the radix select of a frame with 0 < k < count finds"""
    lo, hi = int(offsets[f]), int(offsets[f + 1])
    assert 0 < k[f] < hi - lo
    return int(np.sort(ordered_key(logits[lo:hi]))[::-1][k[f] - 1])


TK_TILE = 2048


def four_launches(counts):
    """The host's choice between the two placement forms, restated from pcc_topk_prune_map (topk.hip, `tiles` and
    the condition under it): flags + one scan of 2n words + emit iff the longest frame has more than 2048 tiles of
    2048 rows, or the per-frame tile sums [frames][tiles][2] would not fit the 2n-word flag array they live in."""
    n, max_cnt = int(sum(counts)), int(max(counts))
    assert n > 0
    tiles = max(1, -(-max_cnt // TK_TILE))
    return max_cnt > TK_TILE * TK_TILE or len(counts) * tiles > n


def staged(counts):
    """more than 8 frames: per-frame parameters through pinned staging instead of kernel arguments (TOPK_ARG_FRAMES)"""
    return len(counts) > 8


# ------------------------------------------------------------------ the byte alphabet and the digit-edge sweep
ALPHABET_BYTES = (0x00, 0x01, 0x80, 0xFF)
SWEEP_ROWS, SWEEP_FRAMES = 3000, 8


@functools.lru_cache(maxsize=None)
def alphabet_keys():
    """the 256 keys whose four bytes each come from {0x00, 0x01, 0x80, 0xFF}"""
    b = np.array(ALPHABET_BYTES, dtype=np.uint32)
    k = (b[:, None, None, None] << 24) | (b[None, :, None, None] << 16) | (b[None, None, :, None] << 8) | b[None, None, None, :]
    return np.sort(k.reshape(-1).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def sweep_frame():
    """3000 rows drawn with replacement from the alphabet: (logits [3000], keys [3000])"""
    rng = np.random.default_rng(20240)
    keys = alphabet_keys()[rng.integers(0, 256, SWEEP_ROWS)]
    return float_from_key(keys), keys


@functools.lru_cache(maxsize=None)
def sweep_classes():
    """distinct keys of the sweep frame from the top, their sizes, and the cumulative counts c_i from the top"""
    _, keys = sweep_frame()
    uk, cnt = np.unique(keys, return_counts=True)
    uk, cnt = uk[::-1], cnt[::-1]
    return uk, cnt, np.cumsum(cnt)


@functools.lru_cache(maxsize=None)
def sweep_ks():
    """every class boundary c_i - 1, c_i, c_i + 1 with c_0 = 0 (c_256 + 1 = 3001: more than the frame holds),
    ascending"""
    cum = np.concatenate([[0], sweep_classes()[2]])
    ks = np.unique(np.concatenate([cum - 1, cum, cum + 1]))
    return [int(v) for v in ks if 0 <= v <= SWEEP_ROWS + 1]


def sweep_threshold(k):
    """threshold key of the sweep frame for 0 < k < 3000"""
    _, keys = sweep_frame()
    return int(np.sort(keys)[::-1][k - 1])


@functools.lru_cache(maxsize=None)
def sweep_calls():
    """The sweep as calls of 8 frames, each frame the same logits with another k: [(logits, offsets, k), ...]; the
    last call is filled up with the last k."""
    lg, _ = sweep_frame()
    ks = sweep_ks()
    ks = ks + [ks[-1]] * (-len(ks) % SWEEP_FRAMES)
    logits = np.ascontiguousarray(np.tile(lg, SWEEP_FRAMES))
    offs = offsets_of([SWEEP_ROWS] * SWEEP_FRAMES)
    return [(logits, offs, ks[i:i + SWEEP_FRAMES]) for i in range(0, len(ks), SWEEP_FRAMES)]


# ------------------------------------------------------------------ named special-value frames
def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


POS_NANS = (0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FC12345, 0x7FA00000)
NEG_NANS = (0xFFC00000, 0xFF800001, 0xFFFFFFFF, 0xFFC12345)


@functools.lru_cache(maxsize=None)
def special(name):
    """(logits, offsets, k, thr): thr[f] = the key the threshold of frame f must have (checked on the CPU by the test
    that uses the case), None where the frame is there for its values alone"""
    rng = np.random.default_rng(sorted(SPECIAL).index(name) + 100)
    if name == "neg_inf_mask":
        # two thirds of the logits masked with -inf, k beyond the finite rows: the threshold is -inf, ties by row
        counts = [3000, 2500]
        lg = rng.normal(size=sum(counts)).astype(np.float32)
        lg[rng.random(lg.shape[0]) < 2 / 3] = -np.inf
        offs = offsets_of(counts)
        fin = [int(np.isfinite(lg[offs[f]:offs[f + 1]]).sum()) for f in range(2)]
        k = [fin[0] + 200, fin[1] + 1]
        thr = [0x007FFFFF, 0x007FFFFF]
    elif name == "pos_inf":
        counts = [3000, 2500]
        lg = rng.normal(size=sum(counts)).astype(np.float32)
        lg[rng.random(lg.shape[0]) < 0.2] = np.inf
        offs = offsets_of(counts)
        inf = [int(np.isposinf(lg[offs[f]:offs[f + 1]]).sum()) for f in range(2)]
        k = [inf[0] - 100, inf[1] - 1]
        thr = [0xFF800000, 0xFF800000]
    elif name == "plus_zero":
        # frame 0: threshold +0.0 among the +0.0 rows, every -0.0 row loses; frame 1: threshold -0.0, every +0.0 kept
        counts = [3000, 3000]
        one = np.concatenate([np.abs(rng.normal(size=700)) + 1e-3, np.zeros(800), -np.zeros(800),
                              -np.abs(rng.normal(size=700)) - 1e-3]).astype(np.float32)
        lg = np.concatenate([rng.permutation(one), rng.permutation(one)])
        k = [700 + 400, 700 + 800 + 300]
        thr = [0x80000000, 0x7FFFFFFF]
    elif name == "denormals":
        # denormals of both signs and both zeros: float bits 0 ... 63 with a random sign
        counts = [3000, 2000]
        bits = rng.integers(0, 64, sum(counts)).astype(np.uint32) | (rng.integers(0, 2, sum(counts)).astype(np.uint32) << 31)
        lg = _f32(bits)
        k = [1000, 1999]
        thr = [None, None]
    elif name == "nans":
        # NaNs of both signs and several payloads and both infinities among finite values; frame 0's threshold is
        # a positive NaN (above +inf), frame 1's a negative one (below -inf)
        counts = [3000, 3000]
        pool = np.concatenate([_f32(POS_NANS), _f32(NEG_NANS), np.array([np.inf, -np.inf], np.float32)])
        lg = rng.normal(size=sum(counts)).astype(np.float32)
        where = rng.random(lg.shape[0]) < 0.3
        lg[where] = pool[rng.integers(0, pool.shape[0], int(where.sum()))]
        offs = offsets_of(counts)
        pos = int((ordered_key(lg[:3000]) > 0xFF800000).sum())
        neg = int((ordered_key(lg[3000:]) < 0x007FFFFF).sum())
        k = [pos // 2, 3000 - neg // 2]
        thr = [None, None]
    elif name == "dense_last_byte":
        counts = [3000, 1000]
        keys = np.uint32(0xBF123400) | rng.integers(0, 256, sum(counts)).astype(np.uint32)
        lg = float_from_key(keys)
        k = [1000, 999]
        thr = [None, None]
    elif name == "top_byte_only":
        counts = [3000, 1000]
        keys = (rng.integers(0, 256, sum(counts)).astype(np.uint32) << 24) | np.uint32(0x00ABCDEF)
        lg = float_from_key(keys)
        k = [1234, 1]
        thr = [None, None]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(lg, dtype=np.float32), offsets_of(counts), k, thr


SPECIAL = ("neg_inf_mask", "pos_inf", "plus_zero", "denormals", "nans", "dense_last_byte", "top_byte_only")


# ------------------------------------------------------------------ frames with spread keys (sequences, frame counts)
def spread(seed, counts, kfrac=None):
    """(logits, offsets, k): half the frames normal() draws, half sixteenths (ties), 0 < k < count wherever the frame has
    two rows or more"""
    rng = np.random.default_rng(seed)
    parts, k = [], []
    for f, c in enumerate(counts):
        if f % 2:
            parts.append((rng.integers(-2000, 2000, c) / 16).astype(np.float32))
        else:
            parts.append((rng.normal(size=c) * 3).astype(np.float32))
        frac = rng.uniform(0.1, 0.9) if kfrac is None else kfrac
        k.append(min(max(1, int(c * frac)), max(c - 1, 0)))
    lg = np.concatenate(parts) if parts else np.empty(0, np.float32)
    return np.ascontiguousarray(lg, dtype=np.float32), offsets_of(counts), k


# ------------------------------------------------------------------ both placement forms
@functools.lru_cache(maxsize=None)
def tiny(name):
    """(logits, offsets, k, four): few rows in many frames; k of 0, 1 and count among them"""
    rng = np.random.default_rng(sorted(TINY).index(name) + 200)
    if name == "1_0_0_2":
        counts, k = [1, 0, 0, 2], [1, 0, 3, 1]
    elif name == "0_0_0_0_0_1":
        counts, k = [0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 1, 1]
    elif name == "12_frames_7_rows":
        counts = [0, 2, 0, 1, 0, 0, 3, 0, 0, 1, 0, 0]
        k = [0, 1, 1, 0, 0, 2, 1, 0, 0, 1, 0, 0]
    elif name == "120_frames_100_rows":
        counts = [0] * 120
        for f in rng.integers(0, 120, 100):
            counts[int(f)] += 1
        k = [[0, 1, c][i % 3] for i, c in enumerate(counts)]
    elif name == "4_frames_4_rows":
        counts, k = [1, 1, 1, 1], [1, 0, 1, 1]
    elif name == "4_frames_3_rows":
        counts, k = [1, 1, 0, 1], [1, 0, 1, 1]
    else:
        raise KeyError(name)
    lg = rng.integers(-3, 3, sum(counts)).astype(np.float32)
    four = name != "4_frames_4_rows"
    return lg, offsets_of(counts), k, four


TINY = ("1_0_0_2", "0_0_0_0_0_1", "12_frames_7_rows", "120_frames_100_rows", "4_frames_4_rows", "4_frames_3_rows")

LARGE = {"4194304": 2048 * 2048, "4194305": 2048 * 2048 + 1}


@functools.lru_cache(maxsize=None)
def large(name):
    """(logits, offsets, k, four): one frame on either side of the 2048 x 2048 switch plus a 300-row frame, tie-heavy"""
    counts = [LARGE[name], 300]
    rng = np.random.default_rng(LARGE[name])
    lg = (rng.integers(-50, 50, sum(counts)) / 8).astype(np.float32)
    return lg, offsets_of(counts), [counts[0] // 3, 100], name == "4194305"


# ------------------------------------------------------------------ frame-count edges
@functools.lru_cache(maxsize=None)
def nine_frames():
    return spread(41, [2500, 1, 3000, 0, 2048, 2049, 700, 4097, 1300])


@functools.lru_cache(maxsize=None)
def many_frames():
    """120 frames, empty ones among them, two launches with staged parameters"""
    rng = np.random.default_rng(42)
    counts = [int(c) for c in rng.integers(0, 200, 120)]
    for f in (0, 7, 8, 64, 119):
        counts[f] = 0
    return spread(43, counts)


@functools.lru_cache(maxsize=None)
def oversized_k():
    """k beyond the frame, 2**40 among them, next to one frame that selects"""
    lg, offs, k = spread(44, [3000, 1, 2500, 700, 0])
    return lg, offs, [3001, 2 ** 40, k[2], 2 * 700, 5]


# ------------------------------------------------------------------ every input set of this file
def all_inputs(with_large=True):
    """(name, logits, offsets, k) of every case above"""
    for i, (lg, offs, k) in enumerate(sweep_calls()):
        yield "sweep%d" % i, lg, offs, k
    for name in SPECIAL:
        yield (name,) + special(name)[:3]
    for name in TINY:
        yield (name,) + tiny(name)[:3]
    yield ("nine_frames",) + nine_frames()
    lg, offs, k = nine_frames()
    yield "eight_frames", lg[:offs[8]], offs[:9], k[:8]
    yield ("many_frames",) + many_frames()
    yield ("oversized_k",) + oversized_k()
    for step, counts in enumerate(SEQUENCE):
        if counts is not None and sum(counts):
            yield ("sequence%d" % step,) + sequence_call(step)
    if with_large:
        for name in LARGE:
            yield (name,) + large(name)[:3]


# The call sequence on one runtime: frame counts per call (None: the call with n == 0).  8 frames use both histogram
# buffers of the context in turn and all of their words; 9 frames go through staging and leave the buffers alone; the tiny
# call takes the four-launch form, whose last launch clears the other buffer as well.
SEQ8 = [3000, 2500, 4100, 2048, 2049, 3500, 2600, 5000]
SEQUENCE = [SEQ8, SEQ8, [3000], None, SEQ8 + [2700], SEQ8, [1, 0, 0, 2], SEQ8, SEQ8, SEQ8]
SEQ_NO_SELECT = 8


def sequence_call(step):
    """fresh seeded data for call `step` of SEQUENCE"""
    counts = SEQUENCE[step]
    if counts is None:
        return np.empty(0, np.float32), [0, 0], [5]
    lg, offs, k = spread(300 + step, counts)
    if step == SEQ_NO_SELECT:                     # no frame selects: every k is 0 or at least the frame
        k = [0 if f % 2 else counts[f] + f for f in range(len(counts))]
    if counts == [1, 0, 0, 2]:
        k = [1, 0, 0, 1]
    return lg, offs, k
