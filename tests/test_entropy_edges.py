"""Entropy kernels (csrc/entropy.hip) at the shapes, table lengths, ties and int16 boundaries they decide on, against
the CPU oracle.  The oracle takes c from the array shapes and its tables from oracle.t[...]: tables and medians of
other lengths are swapped in for the length of a comparison.  Every comparison is equality of integers or of
float32 bit patterns; symbols stay within int32 except where a test says otherwise."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TABLE, MEDIANS = "gaussian_conditional.scale_table", "entropy_bottleneck.medians"


def dev(rt, a):
    return rt.to_device(np.ascontiguousarray(a))


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@contextlib.contextmanager
def swapped(oracle, key, value):
    saved = oracle.t[key]
    try:
        oracle.t[key] = value
        yield
    finally:
        oracle.t[key] = saved


def model_table(oracle):
    return np.ascontiguousarray(oracle.t[TABLE], dtype=np.float32)


def inputs(rng, n, c):
    y = (rng.normal(size=(n, c)) * 2).astype(np.float32)
    params = np.concatenate([np.abs(rng.normal(1.5, 3.0, (n, c))), rng.normal(0, 1, (n, c))], 1).astype(np.float32)
    params[0, 0] = -1.0                       # below the lower bound
    params[n - 1, c - 1] = 1000.0             # above the table
    return y, params


def hold_gaussian(rt, oracle, y, params, scale, tab_h):
    """every Gaussian entry point on one input against the oracle (whose table is tab_h at this moment)"""
    nq = scale.shape[0]
    tab = dev(rt, tab_h)
    dy, dp, ds = dev(rt, y), dev(rt, params), dev(rt, scale)
    rs, ri = oracle.gaussian_quant(y, params, scale)
    sym, idx = rt.gaussian_quant(dy, dp, ds, tab)
    assert np.array_equal(host(sym), rs) and np.array_equal(host(idx), ri)
    s16, i8, flag = rt.gaussian_quant16(dy, dp, ds, tab)
    assert int(flag.item()) == 0
    assert np.array_equal(host(s16).astype(np.int32), rs) and np.array_equal(host(i8).astype(np.int32), ri)
    sd, id8 = rt.gaussian_quant_dev(dy, dp, ds, tab)
    assert sd.dtype == torch.int32 and id8.dtype == torch.uint8
    assert np.array_equal(host(sd), rs) and np.array_equal(host(id8).astype(np.int32), ri)
    for q in range(nq):
        want = oracle.gaussian_indexes(params, scale[q])
        assert np.array_equal(want, ri[q])
        assert np.array_equal(host(rt.gaussian_indexes(dp, dev(rt, scale[q]), tab)), want)
        assert np.array_equal(host(rt.gaussian_indexes8(dp, dev(rt, scale[q]), tab)).astype(np.int32), want)
        yh = rt.gaussian_dequant(dev(rt, rs[q]), dp, dev(rt, scale[q]), float(tab_h[0]), float(oracle.off_a),
                                 float(oracle.off_b))
        assert np.array_equal(bits(host(yh)), bits(oracle.gaussian_dequant(rs[q], params, scale[q])))


# ------------------------------------------------------------------ shapes
NS, CS = (1, 15, 16, 17, 33, 257), (1, 3, 63, 64, 65, 200, 256)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_shape_grid(rt, oracle, n, c):
    """rows around the 16-row tile, channels around the 64 lanes of a wave and at the 256-channel limit; one and three
    qualities with random scales, and three with power-of-two scales (every product exact)"""
    rng = np.random.default_rng(1000 * n + c)
    y, params = inputs(rng, n, c)
    tab_h = model_table(oracle)
    for nq, kind in ((1, "random"), (3, "random"), (3, "pow2")):
        if kind == "random":
            scale = rng.uniform(0.3, 4.0, (nq, c)).astype(np.float32)
        else:
            scale = (2.0 ** rng.integers(-2, 3, (nq, c))).astype(np.float32)
        hold_gaussian(rt, oracle, y, params, scale, tab_h)
    med = rng.normal(0, 2, c).astype(np.float32)
    z = (rng.normal(size=(n, c)) * 3).astype(np.float32)
    z[0, :] = np.float32(0.5) + np.rint(med)             # exact ties wherever the median is an integer
    med[::2] = np.rint(med[::2])
    with swapped(oracle, MEDIANS, med):
        rs, rz = oracle.factorized_quant(z)
        back = oracle.factorized_dequant(rs)
    sym, zhat = rt.factorized_quant(dev(rt, z), dev(rt, med))
    assert np.array_equal(host(sym), rs) and np.array_equal(bits(host(zhat)), bits(rz))
    assert np.array_equal(bits(host(rt.factorized_dequant(sym, dev(rt, med)))), bits(back))


# ------------------------------------------------------------------ table lengths
def sub_table(table, n_tab):
    """ascending sub-sample of the model's 64-entry table that keeps its first and last entry"""
    pick = np.unique(np.rint(np.linspace(0, table.shape[0] - 1, n_tab)).astype(np.int64))
    assert pick.shape[0] == n_tab
    return np.ascontiguousarray(table[pick])


def table_scales(rng, tab_h, n, c):
    """params whose scale column 0 ties with every table entry, column 1 lies below table[0] (negative and zero among
    them), column 2 above the last entry, with NaN and inf in column 3; the rest random over the table's range"""
    y, params = inputs(rng, n, c)
    params[:, :c] = rng.uniform(0.0, float(tab_h[-1]) * 1.2, (n, c)).astype(np.float32)
    params[:tab_h.shape[0], 0] = tab_h
    params[tab_h.shape[0]:2 * tab_h.shape[0], 0] = np.nextafter(tab_h, np.float32(np.inf))
    params[2 * tab_h.shape[0]:3 * tab_h.shape[0], 0] = np.nextafter(tab_h, np.float32(-np.inf))
    params[:, 1] = np.linspace(-1.0, float(tab_h[0]), n).astype(np.float32)
    params[3, 1] = 0.0
    params[:, 2] = (float(tab_h[-1]) * rng.uniform(1.0, 50.0, n)).astype(np.float32)
    params[0, 2] = np.nextafter(tab_h[-1], np.float32(np.inf))
    params[0:6, 3] = np.nan
    params[6:9, 3] = np.inf
    params[9:11, 3] = -np.inf
    return y, params


@pytest.mark.parametrize("n_tab", [2, 3, 63, 64])
def test_table_lengths(rt, oracle, n_tab):
    rng = np.random.default_rng(n_tab)
    tab_h = sub_table(model_table(oracle), n_tab)
    assert np.all(np.diff(tab_h) > 0)
    n, c = 200, 5
    y, params = table_scales(rng, tab_h, n, c)
    one = np.ones((1, c), dtype=np.float32)                 # scale 1.0 keeps the ties exact
    with swapped(oracle, TABLE, tab_h):
        hold_gaussian(rt, oracle, y, params, one, tab_h)
        want = oracle.gaussian_indexes(params, one[0])
        assert want.min() == 0 and want.max() == n_tab - 1
        # the element-wise form on the same scales: the oracle with one channel per element column
        flat = np.ascontiguousarray(params[:, :c].T).reshape(-1)
        two = np.stack([flat, np.zeros_like(flat)], 1)
        ref = oracle.gaussian_indexes(two, np.ones(1, np.float32))[0]
    assert np.array_equal(ref, want.reshape(-1))
    # ... and the definition written out: idx = (n_tab - 1) - #{j < n_tab - 1 : max(s, table[0]) <= table[j]}
    s = np.where(flat > tab_h[0], flat, tab_h[0])
    assert np.array_equal((n_tab - 1) - (s[:, None] <= tab_h[None, :-1]).sum(1), ref)
    got = rt.build_indexes(dev(rt, flat), dev(rt, tab_h))
    assert np.array_equal(host(got), ref)


# ------------------------------------------------------------------ ties and the zero bin
HALF_EVEN = {-3: -2, -2: -2, -1: 0, 0: 0, 1: 2, 2: 2, 3: 4}     # rint(m + 0.5), written out


def test_quantiser_ties_round_half_to_even(rt, oracle):
    """y*s - mu*s exactly m + 0.5 for m = -3 ... 3, with scales 1.0 and 0.5 (both products exact)"""
    ms = np.arange(-3, 4)
    scale = np.array([[1.0, 1.0, 0.5, 0.5, 1.0]], dtype=np.float32)
    mus = np.array([0.0, 2.0, 0.0, -4.0, 1024.0], dtype=np.float32)
    n, c = ms.shape[0], scale.shape[1]
    y = np.empty((n, c), np.float32)
    for ch in range(c):
        y[:, ch] = (ms + 0.5) / scale[0, ch] + mus[ch]
    params = np.concatenate([np.ones((n, c), np.float32), np.tile(mus, (n, 1))], 1).astype(np.float32)
    d = (y.astype(np.float64) * scale) - (params[:, c:].astype(np.float64) * scale)
    assert np.array_equal(d, np.tile((ms + 0.5)[:, None], (1, c)))
    want = np.tile(np.array([HALF_EVEN[int(m)] for m in ms], np.int32)[None, :], (c, 1))[None]     # [1, c, n]
    tab = dev(rt, model_table(oracle))
    args = (dev(rt, y), dev(rt, params), dev(rt, scale), tab)
    assert np.array_equal(host(rt.gaussian_quant(*args)[0]), want)
    s16, _, flag = rt.gaussian_quant16(*args)
    assert int(flag.item()) == 0 and np.array_equal(host(s16).astype(np.int32), want)
    assert np.array_equal(host(rt.gaussian_quant_dev(*args)[0]), want)
    assert np.array_equal(oracle.gaussian_quant(y, params, scale)[0], want)
    # the element-wise form and the factorized quantiser on the same ties
    x = (ms + 0.5).astype(np.float32)
    assert np.array_equal(host(rt.quantize_symbols(dev(rt, x))), want[0, 0])
    assert np.array_equal(host(rt.quantize_symbols(dev(rt, x + np.float32(2.0)), dev(rt, np.full(n, 2.0, np.float32)))),
                          want[0, 0])
    sym, zhat = rt.factorized_quant(dev(rt, y[:, :2]), dev(rt, mus[:2]))
    assert np.array_equal(host(sym), want[0, :2])
    assert np.array_equal(bits(host(zhat)), bits(want[0, :2].T.astype(np.float32) + mus[None, :2]))


def test_dequantiser_zero_bin_sign_and_bound(rt, oracle):
    """symbols 0, +-1, +-2, the int16 limits and +-(2**24 + 1) (not a float32) with sigma below, at and above the bound"""
    syms = np.array([0, 1, -1, 2, -2, 32767, -32768, 2 ** 24 + 1, -(2 ** 24 + 1)], dtype=np.int32)
    tab_h = model_table(oracle)
    bound = tab_h[0]
    sig = np.array([-1.0, 0.0, bound / 2, np.nextafter(bound, np.float32(0)), bound, np.nextafter(bound, np.float32(1)),
                    bound * 2, 7.5], dtype=np.float32)
    rng = np.random.default_rng(5)
    c = 3
    scale = np.array([1.0, 0.5, 1.7], dtype=np.float32)
    n = syms.shape[0] * sig.shape[0]
    params = np.empty((n, 2 * c), np.float32)
    params[:, :c] = np.repeat(sig, syms.shape[0])[:, None] / np.array([1.0, 0.5, 1.0], np.float32)[None, :]
    mu = rng.normal(0, 1, (syms.shape[0], c)).astype(np.float32)            # one mean per symbol, the same for every sigma
    mu[:, 0] = 0.0                                         # mu = 0: the sign of a zero result is the kernel's own
    params[:, c:] = np.tile(mu, (sig.shape[0], 1))
    sym = np.ascontiguousarray(np.tile(np.tile(syms, sig.shape[0])[None, :], (c, 1)))      # [c, n]
    want = oracle.gaussian_dequant(sym, params, scale)
    got = rt.gaussian_dequant(dev(rt, sym), dev(rt, params), dev(rt, scale), float(bound), float(oracle.off_a),
                              float(oracle.off_b))
    assert np.array_equal(bits(host(got)), bits(want))
    zero = np.tile(syms, sig.shape[0]) == 0
    assert np.array_equal(bits(want[zero]), bits(params[zero, c:]))          # the zero bin decodes to mu, no offset
    # sigma below the bound decodes as the bound itself does (channels 0 and 1: sigma = column * scale is exact), a
    # sigma above it does not
    rows = syms.shape[0]
    assert np.array_equal(params[:rows * sig.shape[0], :2] * scale[None, :2], np.repeat(sig, rows)[:, None] * np.ones((1, 2), np.float32))
    at = bits(want[4 * rows:5 * rows, :2])
    for j in (0, 1, 2, 3):
        assert np.array_equal(bits(want[j * rows:(j + 1) * rows, :2]), at)
    assert not np.array_equal(bits(want[6 * rows:7 * rows, :2]), at)


# ------------------------------------------------------------------ the int16 flag
@pytest.mark.parametrize("where", ["first", "last_of_partial_tile", "beyond_256_in_tile"])
def test_int16_flag_boundaries(rt, oracle, where):
    """one element at the int16 limits (flag 0) and one past them or NaN (flag 1), everything else small"""
    n, c = 37, 65                                          # tiles of 16 rows: the last one has 5
    r, ch = {"first": (0, 0), "last_of_partial_tile": (n - 1, c - 1), "beyond_256_in_tile": (21, 40)}[where]
    if where == "beyond_256_in_tile":
        assert ch * 16 + (r % 16) > 256                    # element index within the tile: a thread's second turn or later
    rng = np.random.default_rng(r * 100 + ch)
    base = rng.integers(-300, 300, (n, c)).astype(np.float32)
    params = np.concatenate([np.ones((n, c), np.float32), np.zeros((n, c), np.float32)], 1)
    scale = np.ones((1, c), np.float32)
    tab = dev(rt, model_table(oracle))
    for v, flagged in ((32767.0, 0), (-32768.0, 0), (32768.0, 1), (-32769.0, 1), (np.nan, 1)):
        y = base.copy()
        y[r, ch] = v
        s16, i8, flag = rt.gaussian_quant16(dev(rt, y), dev(rt, params), dev(rt, scale), tab)
        assert int(flag.item()) == flagged, v
        y_ref = y.copy()
        if flagged:
            y_ref[r, ch] = 0.0                             # outside int16 the element is compared by the flag alone
        rs, ri = oracle.gaussian_quant(y_ref, params, scale)
        keep = np.ones((1, c, n), bool)
        keep[0, ch, r] = not flagged
        assert np.array_equal(host(s16)[keep], rs.astype(np.int16)[keep])
        assert np.array_equal(host(s16).astype(np.int32)[keep], rs[keep])
        assert np.array_equal(host(i8).astype(np.int32), ri)


# ------------------------------------------------------------------ element-wise forms
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_quantize_symbols(rt, oracle, n):
    """round(x - means) and round(x) element-wise == the oracle's Gaussian quantiser at c = 1, scale 1.0 (x * 1.0 and
    means * 1.0 are exact), == the definition in numpy float32"""
    rng = np.random.default_rng(n)
    x = (rng.normal(size=n) * 40).astype(np.float32)
    means = rng.normal(0, 3, n).astype(np.float32)
    x[::5] = np.rint(x[::5]) + np.float32(0.5)             # ties, also after the subtraction of an integer mean
    means[::10] = np.rint(means[::10])
    x[-1] = -0.25                                          # rounds to -0.0
    one = np.ones((1, 1), np.float32)
    for m in (means, None):
        mu = means if m is not None else np.zeros(n, np.float32)
        params = np.stack([np.ones(n, np.float32), mu], 1)
        ref = oracle.gaussian_quant(x[:, None], params, one)[0][0, 0]
        assert np.array_equal(ref, np.rint(x - mu).astype(np.int32))
        got = rt.quantize_symbols(dev(rt, x), dev(rt, m) if m is not None else None)
        assert got.dtype == torch.int32 and np.array_equal(host(got), ref)
