"""The interleaved rANS stream of container version 1 on the CPU: tests/rans_il_ref.py (numpy, arbitrary tables, any T,
damaged streams) against the C oracle byte for byte and symbol for symbol; the premise of the GPU encoder's division
(one float32 multiplication by 1 / freq, corrected by one either way) against exact integer division; and the header
bounds pcc_rans_stream_info checks on the host.  tests/test_gpu_rans_edges.py takes the same reference to the GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

import rans_il_ref as R
from conftest import pkg

NS = [0, 1, 64, 65, 4099, 32768, 32769, 70001]


def _tables(oracle, which):
    return R.edge_tables() if which == "edge" else oracle._tables(which)


@pytest.mark.parametrize("with_run", [False, True], ids=["idx", "idx_run"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("which", ["gaussian_conditional", "entropy_bottleneck", "edge"])
def test_reference_equals_oracle(oracle, which, n, with_run):
    tables = _tables(oracle, which)
    run = max(-(-n // len(tables[1])), 1) if with_run else 0
    sym, idx = R.plain_case(np.random.default_rng(n + 7), n, tables, run)
    run = run or 1
    data = R.encode(sym, idx, tables, idx_run=run)
    assert data == R.oracle_encode(oracle, sym, idx, tables, idx_run=run)
    hn, T, words = R.header(data)
    assert (hn, T, len(words)) == (n, R.steps_for(n), R.chunks_for(n, R.steps_for(n)))
    assert np.array_equal(R.decode(data, idx, n, tables, idx_run=run), sym)
    rc, back = R.oracle_decode_rc(oracle, data, idx, n, tables, idx_run=run)
    assert rc == 0 and np.array_equal(back, sym)


def test_reference_on_the_edge_specials(oracle):
    """every row's v0 in {-1, 0, max - 1, max}, escapes of every nibble count, INT32_MAX / INT32_MIN on offset-0 rows"""
    tables = R.edge_tables()
    sym, idx = R.edge_case(np.random.default_rng(1), 4099, tables)
    assert R.nibble_counts(sym, idx, tables) == set(range(9))
    v0 = sym.astype(np.int64) - tables[2][idx]
    assert v0.max() == 2 ** 31 - 1 and v0.min() == -2 ** 31
    data = R.encode(sym, idx, tables)
    assert data == R.oracle_encode(oracle, sym, idx, tables)
    assert np.array_equal(R.decode(data, idx, sym.shape[0], tables), sym)


def test_all_frequency_one_input_costs_one_word_per_symbol():
    """what the capacity cases of the GPU file build on"""
    tables = R.edge_tables()
    rng = np.random.default_rng(2)
    n = 512
    sym = (rng.integers(0, 1000, n) + tables[2][R.ROW_B]).astype(np.int32)
    _, _, words = R.header(R.encode(sym, np.full(n, R.ROW_B, dtype=np.uint8), tables))
    assert list(words) == [2 * 64 + n]


@pytest.mark.parametrize("T,n", [(1, 64 * 3000), (7, 64 * 7 * 4 + 1), (9, 64 * 9 * 5), (513, 64 * 513 - 63), (513, 64 * 513 * 2 + 1),
                                 (1000, 64000), (1000, 64000 * 2 + 77)])
def test_forced_steps_per_chunk(oracle, T, n):
    tables = R.edge_tables()
    sym, idx = R.plain_case(np.random.default_rng(T), n, tables)
    data = R.encode(sym, idx, tables, T=T)
    hn, hT, words = R.header(data)
    assert (hn, hT, len(words)) == (n, T, -(-n // (64 * T)))
    assert np.array_equal(R.decode(data, idx, n, tables), sym)
    rc, back = R.oracle_decode_rc(oracle, data, idx, n, tables)      # the oracle's decoder reads T from the header
    assert rc == 0 and np.array_equal(back, sym)


def test_damaged_streams_raise_the_oracles_codes(oracle):
    tables = R.edge_tables()
    n = 300
    sym, idx = R.edge_case(np.random.default_rng(3), n, tables)
    esc = np.flatnonzero(R.lookup(sym, idx.astype(np.int64), tables)[4])
    good = R.encode(sym, idx, tables, T=2)
    cases = [(good[:12], -1), (b"XXXX" + good[4:], -1), (good[:-2], -2), (good + b"\0\0", -2),
             (R.encode(sym, idx, tables, T=2, nibble_count={int(esc[0]): 9}), -3),
             (R.encode(sym, idx, tables, T=2, nibble_count={int(esc[-1]): 15}), -3)]
    # one word moved from chunk 0 to chunk 1: chunk 0 runs out of words
    _, _, words = R.header(good)
    moved = bytearray(good)
    struct.pack_into("<2I", moved, 16, int(words[0]) - 1, int(words[1]) + 1)
    cases.append((bytes(moved), -2))
    for data, code in cases:
        with pytest.raises(R.StreamError) as e:
            R.decode(data, idx, n, tables)
        assert e.value.code == code
        assert R.oracle_decode_rc(oracle, data, idx, n, tables)[0] == code


# ---------------------------------------------------------------------------------- the encoder's division
_quotient_f32 = R.quotient_f32     # the kernel's recipe, restated in float32 numpy


def test_float_reciprocal_quotient_is_within_one_and_its_correction_exact():
    """every freq in 1 .. 65536; x = q freq + r below 2^16 freq (what renormalisation leaves), q at the ends, the byte
    and half-word edges and 40 random places, r at 0, 1, freq - 1, freq / 2 and random"""
    rng = np.random.default_rng(6)
    f = np.arange(1, 65537, dtype=np.int64)
    qs = [0, 1, 2, 255, 256, 4095, 4096, 32767, 32768, 65534, 65535] + [int(v) for v in rng.integers(0, 65536, 40)]
    worst = 0
    for q in qs:
        for r in (np.zeros_like(f), np.minimum(1, f - 1), f - 1, f // 2, rng.integers(0, 1 << 30, f.shape[0]) % f):
            x = q * f + r
            assert x.max() < 2 ** 32
            q0, qd, rem = _quotient_f32(x, f)
            worst = max(worst, int(np.abs(q0.astype(np.int64) - q).max()))
            assert np.array_equal(qd.astype(np.int64), x // f) and np.array_equal(rem.astype(np.int64), x % f)
    assert worst <= 1


def test_float_reciprocal_quotient_where_the_product_wraps():
    """freq = 65536 with x next to 2^32: q0 = 65536, q0 * freq wraps to 0, the `under` branch still lands on the pair"""
    x = np.array([2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 65536, 2 ** 32 - 65537], dtype=np.int64)
    f = np.full(4, 65536, dtype=np.int64)
    q0, qd, rem = _quotient_f32(x, f)
    assert int(q0.max()) == 65536                                     # the wrap does happen
    assert np.array_equal(qd.astype(np.int64), x // f) and np.array_equal(rem.astype(np.int64), x % f)


# ---------------------------------------------------------------------------------- pcc_rans_stream_info
def _fake(n, T, words, magic=R.MAGIC):
    """a stream of zeros with this header and chunk table, as long as the table says"""
    return struct.pack("<4I", magic, n, T, len(words)) + np.asarray(words, dtype=np.uint32).tobytes() + bytes(2 * sum(words))


def _info(data):
    abi = pkg("_abi")
    buf = np.frombuffer(data, dtype=np.uint8)
    n, t, c = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    rc = abi.lib().pcc_rans_stream_info(C.c_void_p(buf.ctypes.data), buf.shape[0], C.byref(n), C.byref(t), C.byref(c))
    return rc, (n.value, t.value, c.value)


def test_stream_info_boundaries():
    abi = pkg("_abi")
    ok, bad = abi.PCC_OK, abi.PCC_E_STREAM
    # T at 0, 1, 65536, 65537
    assert _info(_fake(1, 0, [128]))[0] == bad
    assert _info(_fake(64, 1, [128])) == (ok, (64, 1, 1))
    assert _info(_fake(100, 65536, [128])) == (ok, (100, 65536, 1))
    assert _info(_fake(100, 65537, [128]))[0] == bad
    assert b"65537" in abi.lib().pcc_last_error()
    # a chunk count one more and one fewer than n needs (200 symbols, T = 1: four chunks)
    assert _info(_fake(200, 1, [128] * 4)) == (ok, (200, 1, 4))
    assert _info(_fake(200, 1, [128] * 5))[0] == bad
    assert _info(_fake(200, 1, [128] * 3))[0] == bad
    assert _info(_fake(256, 1, [128] * 4)) == (ok, (256, 1, 4))         # n an exact multiple of 64 T
    assert _info(_fake(257, 1, [128] * 4))[0] == bad
    # an empty stream is one chunk of final states
    assert _info(_fake(0, 1, [128])) == (ok, (0, 1, 1))
    assert _info(_fake(0, 1, [128, 128]))[0] == bad
    assert _info(_fake(0, 1, []))[0] == bad
    # a chunk holds at least its 64 states
    assert _info(_fake(64, 1, [127]))[0] == bad
    assert b"no states" in abi.lib().pcc_last_error()
    assert _info(_fake(130, 1, [128, 127, 128]))[0] == bad
    # the chunk table must add up to the length, to the byte
    good = _fake(130, 1, [128, 129, 128])
    assert _info(good) == (ok, (130, 1, 3))
    assert _info(good + b"\0\0")[0] == bad and _info(good[:-2])[0] == bad and _info(good[:24])[0] == bad
    assert _info(_fake(64, 1, [128], magic=R.MAGIC ^ 1))[0] == bad


def test_reference_streams_pass_stream_info(oracle):
    tables = R.edge_tables()
    for T, n in ((None, 4099), (1, 200), (7, 1000), (65536, 100)):
        sym, idx = R.plain_case(np.random.default_rng(n), n, tables)
        data = R.encode(sym, idx, tables, T=T)
        hn, hT, words = R.header(data)
        assert _info(data) == (0, (n, hT, len(words)))
