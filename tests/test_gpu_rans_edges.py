"""The GPU's interleaved rANS coder (csrc/rans_gpu.hip) off the model's tables and off the one layout the encoder
emits: CDF rows at the edges of the search LUT, of the division and of the LDS image; unaligned index arrays; the
status bits only the kernel can raise; steps per chunk no encoder writes; the first attempt's buffer met exactly and
missed by one word; the stream count limit.  Everything goes through runtime.RansDev and is compared exactly — bytes with
the C oracle, symbols with the input, foreign layouts and damaged streams with tests/rans_il_ref.py.  Every case asserts
the property it exists for from its input or from the header the GPU wrote."""
import re
import struct

import numpy as np
import pytest

import rans_il_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def edge(rt):
    tables = R.edge_tables()
    dev = pkg("runtime").RansDev(*tables)
    yield tables, dev
    dev.close()


def _encode(rt, dev, syms, idxs=None, idx_run=1):
    syms = np.ascontiguousarray(np.atleast_2d(syms), dtype=np.int32)
    d_idx = None if idxs is None else rt.to_device(np.ascontiguousarray(np.atleast_2d(idxs), dtype=np.uint8))
    return dev.encode(rt, rt.to_device(syms), d_idx, idx_run)


def _decode(rt, dev, data, n, idx=None, idx_run=1):
    d_idx = None if idx is None or n == 0 else rt.to_device(np.ascontiguousarray(idx, dtype=np.uint8))
    return dev.decode(rt, data, n, d_idx, idx_run).cpu().numpy()


def _both_ways(rt, oracle, dev, tables, sym, idx, idx_run=1):
    """one stream: bytes equal the oracle's, the GPU decodes them to the input; returns the bytes"""
    got = _encode(rt, dev, sym, idx, idx_run)[0]
    assert got == R.oracle_encode(oracle, sym, idx, tables, idx_run)
    assert np.array_equal(_decode(rt, dev, got, sym.shape[0], idx, idx_run), sym)
    return got


def _status(err):
    return int(re.search(r"status (\d+)", str(err)).group(1))


# ---------------------------------------------------------------------------------- 1. edge tables
@pytest.mark.parametrize("n", [1, 64, 65, 4099, 40001])
def test_edge_tables_bytes_and_round_trip(rt, oracle, edge, n):
    """rows A-D and the frequency rows; per row v0 in {-1, 0, max - 1, max} and escapes of every nibble count (all of
    that from n = 4099 on; the nine counts from n = 64 on; n = 1 is one 0-nibble escape on the escape-only row)"""
    tables, dev = edge
    sym, idx = R.edge_case(np.random.default_rng(n), n, tables)
    specials = R.edge_specials(tables)[0].shape[0]
    if n >= 64:
        assert R.nibble_counts(sym, idx, tables) == set(range(9))
    if n >= specials:
        v0 = sym.astype(np.int64) - tables[2][idx]
        assert v0.max() == 2 ** 31 - 1 and v0.min() == -2 ** 31          # on the offset-0 rows
        assert set(idx.tolist()) == set(range(len(tables[1])))
        for raw in R.ESCAPE_RAWS:
            assert R.escape_symbol(raw, R.ROW_C, tables) in sym[idx == R.ROW_C]
    data = _both_ways(rt, oracle, dev, tables, sym, idx)
    assert R.header(data)[1] == R.steps_for(n)


# ---------------------------------------------------------------------------------- 2. frequency sweep
def _sweep_bins(tables):
    """(row, bin, start, freq) of every regular bin of the frequency rows"""
    cdf, sizes, _ = tables
    pairs = [(r, v) for r in range(4, len(sizes)) for v in range(sizes[r] - 2)]
    pr, pv = np.asarray([p[0] for p in pairs]), np.asarray([p[1] for p in pairs])
    return pr, pv, cdf[pr, pv].astype(np.int64), (cdf[pr, pv + 1] - cdf[pr, pv]).astype(np.int64)


def _quotient_misses(sym, idx, tables):
    """how often the float quotient of the encoder is one too small (`over` corrects it) and one too large (`under`)"""
    seen = {"over": 0, "under": 0}

    def trace(x, f):
        q0 = R.quotient_f32(x, f)[0].astype(np.int64)
        seen["over"] += int((q0 < x // f).sum())
        seen["under"] += int((q0 > x // f).sum())
    R.encode(sym, idx, tables, trace=trace)
    return seen["over"], seen["under"]


def _hunted_sweep(tables, n, T=80):
    """symbols of the frequency rows, chosen lane by lane in the encoder's own (backward) order: where some bin makes
    the float quotient of the lane's state miss by one, that bin (a quotient too small first: it is the rare one — a
    uniform draw of 65537 symbols holds none), else a random bin"""
    pr, pv, start, freq = _sweep_bins(tables)
    rng = np.random.default_rng(n)
    pick = np.zeros(n, dtype=np.int64)
    lanes = np.arange(64)
    for c in range(-(-n // (64 * T))):
        x = np.full(64, R.L, dtype=np.int64)
        for t in range(T - 1, -1, -1):
            i = c * 64 * T + t * 64 + lanes
            a = i < n
            if not a.any():
                continue
            xr = np.where(x[:, None] >= (freq[None, :] << 16), x[:, None] >> 16, x[:, None])   # [lane, bin]
            q0 = R.quotient_f32(xr, np.broadcast_to(freq, xr.shape))[0].astype(np.int64)
            q = xr // freq
            k = np.argmax(2.0 * (q0 < q) + 1.0 * (q0 > q) + 0.9 * rng.random(xr.shape), axis=1)
            pick[i[a]] = k[a]
            xk = xr[lanes, k]
            x = np.where(a, ((xk // freq[k]) << 16) + xk % freq[k] + start[k], x)
    idx = pr[pick].astype(np.uint8)
    return (pv[pick] + tables[2][idx]).astype(np.int32), idx


@pytest.fixture(scope="module")
def sweep_inputs():
    tables = R.edge_tables()
    pr, pv, _, freq = _sweep_bins(tables)
    assert set(freq.tolist()) >= set(R.SWEEP_FREQS)
    n = 65537
    rng = np.random.default_rng(n)
    pick = np.concatenate([np.arange(pr.shape[0]), rng.integers(0, pr.shape[0], n - pr.shape[0])])[rng.permutation(n)]
    idx = pr[pick].astype(np.uint8)
    return {n: ((pv[pick] + tables[2][idx]).astype(np.int32), idx), 61441: _hunted_sweep(tables, 61441)}


@pytest.mark.parametrize("n", [65537, 61441])
def test_frequency_sweep(rt, oracle, edge, sweep_inputs, n):
    """bins of frequency 1, 2, 3, 5, 7 and 2^k - 1, 2^k, 2^k + 1 (k = 2 .. 15): the encoder's float quotient and its
    correction at every size of divisor.  T = 80, 13 chunks.  65537 symbols are a uniform draw of the bins; the 61441
    = 12 * 5120 + 1 (the last chunk holds one symbol; 65537 leaves 4097 in it) are hunted for quotients that miss"""
    tables, dev = edge
    sym, idx = sweep_inputs[n]
    assert len(set(zip(idx.tolist(), sym.tolist()))) == _sweep_bins(tables)[0].shape[0]      # every bin occurs
    over, under = _quotient_misses(sym, idx, tables)
    if n == 61441:
        assert over >= 10 and under >= 100, (over, under)                # (the reference counts 16 and 537)
    else:
        assert under >= 10, (over, under)
    data = _both_ways(rt, oracle, dev, tables, sym, idx)
    hn, T, words = R.header(data)
    assert (T, len(words)) == (80, 13)
    if n == 61441:
        assert 128 <= words[-1] <= 129                                    # the states and at most the symbol's word


# ---------------------------------------------------------------------------------- 3. CDF image length
def _random_rows(rng, lengths):
    return [np.concatenate([[0], np.sort(rng.choice(np.arange(1, 65536), k - 2, replace=False)), [65536]]) for k in lengths]


def _all_bins_case(rng, tables, n):
    _, sizes, offsets = tables
    idx = rng.integers(0, len(sizes), n).astype(np.uint8)
    sym = rng.integers(-2, sizes[idx].astype(np.int64) + 1) + offsets[idx]
    last = len(sizes) - 1
    idx[n // 2], sym[n // 2] = last, sizes[last] - 3 + offsets[last]      # the last row's last regular bin
    return sym.astype(np.int32), idx


@pytest.mark.parametrize("lengths", [(2,), (9, 7), (9, 8), (9, 14), (5, 6, 28)])
def test_cdf_image_lengths(rt, oracle, lengths):
    """the table image is staged in 16-byte pieces with a tail: entry counts of 2 and of 0, 1, 7 mod 8, and the last
    row's last regular bin — the image's last two entries — in the input"""
    rng = np.random.default_rng(sum(lengths))
    tables = R.tables_of(_random_rows(rng, lengths), list(range(1, len(lengths) + 1)))
    assert sum(lengths) % 8 == {2: 2, 16: 0, 17: 1, 23: 7, 39: 7}[sum(lengths)]
    dev = pkg("runtime").RansDev(*tables)
    try:
        sym, idx = _all_bins_case(rng, tables, 333)
        _both_ways(rt, oracle, dev, tables, sym, idx)
    finally:
        dev.close()


def _lds_bytes(entries, n_cdf):
    """pcc_rans_dev::lds_bytes: the CDF image padded to 16 B, 3 int32 per row, 65 LUT entries per row"""
    return (entries * 2 + 15) // 16 * 16 + n_cdf * 12 + n_cdf * 65 * 2


def test_largest_table_set_the_lds_admits(rt, oracle):
    runtime = pkg("runtime")
    n_cdf = 8
    entries = max(e for e in range(30000, 34000) if _lds_bytes(e, n_cdf) <= 64 * 1024)
    assert _lds_bytes(entries, n_cdf) == 65536 and entries == 32200
    rng = np.random.default_rng(12)
    lengths = [entries // n_cdf] * (n_cdf - 1) + [entries - entries // n_cdf * (n_cdf - 1)]
    tables = R.tables_of(_random_rows(rng, lengths), list(range(n_cdf)))
    dev = runtime.RansDev(*tables)
    try:
        sym, idx = _all_bins_case(rng, tables, 4099)
        _both_ways(rt, oracle, dev, tables, sym, idx)
    finally:
        dev.close()
    lengths[-1] += 1
    with pytest.raises(runtime.PccError, match=f"{entries + 1} CDF entries do not fit"):
        runtime.RansDev(*R.tables_of(_random_rows(rng, lengths), list(range(n_cdf))))


# ---------------------------------------------------------------------------------- 4. unaligned table indexes
@pytest.mark.parametrize("ns", [(4097, 4098, 4099), (3,)])
def test_unaligned_table_indexes(rt, oracle, edge, ns):
    """stream s of a batch reads its indexes from idx + s n; the decoder from wherever the caller's array starts: both
    fetch the aligned dword around a byte and must pick the byte by the array's misalignment"""
    tables, dev = edge
    seen_enc = set()
    for n in ns:
        cases = [R.edge_case(np.random.default_rng(10 * n + s), n, tables) for s in range(3)]
        d_sym = rt.to_device(np.stack([c[0] for c in cases]))
        d_idx = rt.to_device(np.stack([c[1] for c in cases]))
        assert d_idx.data_ptr() % 4 == 0
        seen_enc |= {(d_idx.data_ptr() + s * n) % 4 for s in range(3)}
        got = dev.encode(rt, d_sym, d_idx)
        for s, (sym, idx) in enumerate(cases):
            assert got[s] == R.oracle_encode(oracle, sym, idx, tables), f"stream {s} of n = {n}"
        sym, idx = cases[1]
        big = rt.empty((n + 16,), torch.uint8)
        assert big.data_ptr() % 4 == 0
        for k in (1, 2, 3):
            view = big[k:k + n]
            view.copy_(torch.from_numpy(idx))
            assert view.data_ptr() % 4 == k
            assert np.array_equal(dev.decode(rt, got[1], n, view, 1).cpu().numpy(), sym), f"n = {n}, offset {k}"
    assert seen_enc >= ({1, 2, 3} if len(ns) == 3 else {2, 3})


# ---------------------------------------------------------------------------------- 5. stream count limit
def test_sixty_four_streams_and_no_more(rt, oracle, edge):
    """the stream lengths come back through 64 slots of the context's pinned block.  No index array (tables by position):
    the streams start at odd offsets, which is case 4's subject"""
    tables, dev = edge
    runtime = pkg("runtime")
    n, rows = 1001, len(tables[1])
    run = -(-n // rows)
    syms = np.stack([R.plain_case(np.random.default_rng(100 + s), n, tables, run)[0] for s in range(65)])
    got = _encode(rt, dev, syms[:64], None, run)
    assert len(set(got)) == 64
    for s in range(64):
        assert got[s] == R.oracle_encode(oracle, syms[s], None, tables, run), f"stream {s}"
    assert np.array_equal(_decode(rt, dev, got[63], n, None, run), syms[63])
    with pytest.raises(runtime.PccError) as e:
        _encode(rt, dev, syms, None, run)
    assert e.value.code == -1
    assert _encode(rt, dev, syms[:1], None, run)[0] == got[0]


# ---------------------------------------------------------------------------------- 6. first-attempt capacity
def _first_attempt_words(T):
    """pcc_rans_encode_dev_async, attempt 0: the states, 1.5 words per symbol, 64 spare"""
    return 2 * 64 + 64 * T * 3 // 2 + 64


def _chunk_of_words(tables, T, target):
    """one chunk of 64 T symbols whose chunk-table entry is exactly `target` words: symbols of frequency 1 (one word
    each), 8-nibble escapes on the escape-only row in place of some (36 bits: two or three words), then single symbols
    traded for row D's near-certain bin (no word)"""
    n = 64 * T
    rng = np.random.default_rng(T)
    offs = tables[2]
    sym = (rng.integers(0, 1000, n) + offs[R.ROW_B]).astype(np.int32)
    idx = np.full(n, R.ROW_B, dtype=np.uint8)
    order = rng.permutation(n)
    n_esc = n_free = 0
    for _ in range(400):
        w = int(R.header(R.encode(sym, idx, tables, T=T))[2][0])
        if w == target:
            return sym, idx
        if w < target:
            k = max((target - w) * 3 // 4 - 2, 1)
            at = order[n_esc:n_esc + k]
            sym[at] = rng.integers(2 ** 28, 2 ** 32, k) // 2          # raw = 2 v0 on row A (max_value 0, offset 0)
            idx[at] = R.ROW_A
            n_esc += k
        else:
            k = w - target
            at = order[n - n_free - k:n - n_free]
            sym[at], idx[at] = offs[R.ROW_D], R.ROW_D
            n_free += k
        assert n_esc + n_free <= n
    raise AssertionError(f"no chunk of {target} words found")


@pytest.fixture(scope="module")
def capacity_inputs():
    """{(T, extra): (sym, idx, chunk)}: T = 8: one chunk, the whole stream.  T = 80 needs more than 32768 symbols, so the
    chunk is the middle one of seven (n = 7 * 5120, the smallest such array), the others cheap"""
    tables = R.edge_tables()
    out = {}
    for extra in (0, 1):
        out[8, extra] = _chunk_of_words(tables, 8, _first_attempt_words(8) + extra) + (0,)
        c_sym, c_idx = _chunk_of_words(tables, 80, _first_attempt_words(80) + extra)
        rng = np.random.default_rng(80 + extra)
        idx = np.full(7 * 5120, R.ROW_C, dtype=np.uint8)
        sym = (rng.integers(0, 64, idx.shape[0]) + tables[2][R.ROW_C]).astype(np.int32)
        sym[3 * 5120:4 * 5120], idx[3 * 5120:4 * 5120] = c_sym, c_idx
        out[80, extra] = (sym, idx, 3)
    return out


def _encode_counting_attempts(rt, dev, syms, idxs):
    rt.prof_enable(True)
    try:
        got = _encode(rt, dev, syms, idxs)
        attempts = [r for r in rt.prof_records() if r[0] == "rans_encode_dev"]
    finally:
        rt.prof_enable(False)
    return got, len(attempts)


@pytest.mark.parametrize("T", [8, 80])
@pytest.mark.parametrize("extra", [0, 1], ids=["exact_fit", "one_word_more"])
def test_first_attempt_capacity(rt, oracle, edge, capacity_inputs, T, extra):
    tables, dev = edge
    sym, idx, chunk = capacity_inputs[T, extra]
    got, attempts = _encode_counting_attempts(rt, dev, sym, idx)
    hn, hT, words = R.header(got[0])
    assert hT == T and len(words) == (1 if T == 8 else 7)
    assert words[chunk] == _first_attempt_words(T) + extra
    assert max(np.delete(words, chunk), default=0) < _first_attempt_words(T) - 64
    assert got[0] == R.oracle_encode(oracle, sym, idx, tables)
    assert attempts == 1 + extra
    assert np.array_equal(_decode(rt, dev, got[0], sym.shape[0], idx), sym)


def test_first_attempt_capacity_in_a_batch(rt, oracle, edge, capacity_inputs):
    """three streams, only the middle one holds the chunk that misses the first buffer by a word: the second attempt
    codes all three again"""
    tables, dev = edge
    sym1, idx1, chunk = capacity_inputs[80, 1]
    rng = np.random.default_rng(5)
    syms, idxs = [], []
    for s in range(3):
        i = np.full(sym1.shape[0], R.ROW_C, dtype=np.uint8)
        syms.append((rng.integers(0, 64, i.shape[0]) + tables[2][R.ROW_C]).astype(np.int32))
        idxs.append(i)
    syms[1], idxs[1] = sym1, idx1
    got, attempts = _encode_counting_attempts(rt, dev, np.stack(syms), np.stack(idxs))
    assert attempts == 2
    for s in range(3):
        assert got[s] == R.oracle_encode(oracle, syms[s], idxs[s], tables), f"stream {s}"
        assert (R.header(got[s])[2].max() > _first_attempt_words(80)) == (s == 1)


# ---------------------------------------------------------------------------------- 7. layouts no encoder emits
LAYOUTS = [(1, 64 * 2999 + 1), (7, 64 * 7 * 4 + 1), (9, 64 * 9 * 5), (513, 64 * 513 - 63), (513, 64 * 513 * 3), (1000, 63999),
           (1000, 64000 * 2 + 1), (65536, 100)]


@pytest.mark.parametrize("T,n", LAYOUTS)
def test_foreign_layouts_decode(rt, edge, T, n):
    """the header carries T and the chunk count and the decoder takes any T in 1 .. 65536: streams of the reference,
    decoded on the GPU.  T = 7 and 9 leave the 8-step unroll with a remainder; n an exact multiple of 64 T (T = 9, 513)
    and a last chunk of one symbol (T = 1, 7, 1000); chunks at odd and at even 16-bit offsets (the parity bit of the
    decoder's window)"""
    tables, dev = edge
    nc = -(-n // (64 * T))
    for seed in range(32):                      # a seed whose chunk table puts chunks at both parities
        sym, idx = R.edge_case(np.random.default_rng(1000 * seed + T), n, tables)
        data = R.encode(sym, idx, tables, T=T)
        hn, hT, words = R.header(data)
        starts = np.concatenate([[0], np.cumsum(words)[:-1]]) % 2
        if nc == 1 or set(starts.tolist()) == {0, 1}:
            break
    assert (hn, hT, len(words)) == (n, T, nc)
    assert nc == 1 or set(starts.tolist()) == {0, 1}
    if n % (64 * T) == 1:
        assert words[-1] <= 128 + 10            # one symbol: the states and at most ten rounds
    assert np.array_equal(_decode(rt, dev, data, n, idx), sym)


def test_foreign_layouts_cover_what_they_claim():
    ts = [t for t, _ in LAYOUTS]
    assert {1, 7, 9, 513, 1000, 65536} == set(ts)
    assert any(n % (64 * t) == 0 and n > 64 * t for t, n in LAYOUTS) and any(n % (64 * t) == 1 and n > 64 * t for t, n in LAYOUTS)
    assert (1, 64 * 2999 + 1) in LAYOUTS and -(-LAYOUTS[0][1] // 64) == 3000
    for t in (513, 1000):
        assert sorted(-(-n // (64 * t)) for tt, n in LAYOUTS if tt == t) == [1, 3]
    for t in (7, 9):
        assert [-(-n // (64 * t)) for tt, n in LAYOUTS if tt == t] == [5]


# ---------------------------------------------------------------------------------- 8. the kernel's own refusals
@pytest.fixture(scope="module")
def refusal_base():
    """300 symbols in three chunks of T = 2; at the first and the last place of every chunk the escape-only row's symbol
    0: an escape of no nibbles, so a forged count changes nothing but the count the decoder reads"""
    tables = R.edge_tables()
    n = 300
    sym, idx = R.edge_case(np.random.default_rng(8), n, tables)
    for at in (0, 127, 128, 255, 256, 299):
        sym[at], idx[at] = 0, R.ROW_A
    return tables, sym, idx, R.encode(sym, idx, tables, T=2)


def _refused(rt, dev, data, n, idx):
    runtime = pkg("runtime")
    with pytest.raises(runtime.PccError) as e:
        _decode(rt, dev, data, n, idx)
    assert e.value.code == -5
    return _status(e.value)


def test_a_chunk_out_of_words_is_status_1(rt, oracle, edge, refusal_base):
    _, dev = edge
    tables, sym, idx, good = refusal_base
    _, _, words = R.header(good)
    for c in (0, 1):
        moved = bytearray(good)
        struct.pack_into("<2I", moved, 16 + 4 * c, int(words[c]) - 1, int(words[c + 1]) + 1)   # total unchanged: the host check passes
        st = _refused(rt, dev, bytes(moved), 300, idx)
        assert st & 1 and not st & 4             # (the chunk behind reads shifted words: it may add bit 2)
        assert R.oracle_decode_rc(oracle, bytes(moved), idx, 300, tables)[0] == -2
    assert np.array_equal(_decode(rt, dev, good, 300, idx), sym)


@pytest.mark.parametrize("count", [9, 15])
@pytest.mark.parametrize("at", [0, 128, 255, 299], ids=["first_of_chunk0", "first_of_chunk1", "last_of_chunk1", "last_of_stream"])
def test_a_nibble_count_above_8_is_status_2(rt, oracle, edge, refusal_base, at, count):
    _, dev = edge
    tables, sym, idx, good = refusal_base
    bad = R.encode(sym, idx, tables, T=2, nibble_count={at: count})
    assert bad != good
    assert _refused(rt, dev, bad, 300, idx) == 2  # the state behind the count is the good stream's: nothing else goes wrong
    assert R.oracle_decode_rc(oracle, bad, idx, 300, tables)[0] == -3
    with pytest.raises(R.StreamError) as e:
        R.decode(bad, idx, 300, tables)
    assert e.value.code == -3
    assert np.array_equal(_decode(rt, dev, good, 300, idx), sym)


@pytest.mark.parametrize("row", ["n_cdf", 255])
@pytest.mark.parametrize("at", [0, 299], ids=["first", "last"])
def test_a_table_index_out_of_range_is_status_4_and_clamped(rt, oracle, edge, refusal_base, at, row):
    """decode reports it; encode codes the symbol with the last row, as include/pcc.h documents"""
    _, dev = edge
    tables, sym, idx, _ = refusal_base
    last = len(tables[1]) - 1
    bad_idx, clamped = idx.copy(), idx.copy()
    bad_idx[at] = last + 1 if row == "n_cdf" else 255
    clamped[at] = last
    want = R.oracle_encode(oracle, sym, clamped, tables)
    assert _encode(rt, dev, sym, bad_idx)[0] == want
    assert _refused(rt, dev, want, 300, bad_idx) == 4
    assert np.array_equal(_decode(rt, dev, want, 300, clamped), sym)


# ---------------------------------------------------------------------------------- 9. idx_run, short last table
def test_tables_by_position_with_a_short_last_run(rt, oracle, edge):
    tables, dev = edge
    rows, run = len(tables[1]), 517
    n = rows * run - 5
    sym, _ = R.plain_case(np.random.default_rng(9), n, tables, run)
    data = _both_ways(rt, oracle, dev, tables, sym, None, run)
    assert R.header(data)[0] == n and (n - 1) // run == rows - 1 and n % run != 0
