"""Top-k pruning (csrc/topk.hip) at the edges it decides on: digit boundaries of the radix select, special values,
both placement forms, the frame counts at which the parameters change their route, the histogram state that outlives
a call, and the refusals.  Inputs and the numpy restatement of the rule: tests/topk_cases.py.  Every comparison is
equality of integers."""
import numpy as np
import pytest

import topk_cases as tc
from conftest import pkg


def dev(rt, a):
    return rt.to_device(np.ascontiguousarray(a))


def host(t):
    return t.cpu().numpy()


_REF = {}


def reference(oracle, name, lg, offs, k):
    """oracle.topk of a named case, computed once"""
    if name not in _REF:
        _REF[name] = oracle.topk(lg, offs, k)
    return _REF[name]


def hold(rt, ref, lg, offs, k, plain=True):
    """kept rows and remap of one call against `ref`"""
    n = lg.shape[0]
    d = dev(rt, lg)
    want_n = sum(min(int(a), offs[f + 1] - offs[f]) for f, a in enumerate(k))
    assert len(ref) == want_n
    if plain:
        keep = rt.topk_prune(d, offs, k)
        assert keep.shape[0] == want_n and np.array_equal(host(keep).view(np.uint32), ref)
    keep, remap = rt.topk_prune(d, offs, k, with_map=True)
    assert keep.shape[0] == want_n and np.array_equal(host(keep).view(np.uint32), ref)
    assert np.array_equal(host(remap), tc.remap_ref(n, ref))


# ------------------------------------------------------------------ the reference and the inputs (no GPU)
def test_key_round_trip_over_the_alphabet():
    keys = tc.alphabet_keys()
    assert keys.shape == (256,) and np.unique(keys).shape == (256,)
    f = tc.float_from_key(keys)
    assert f.dtype == np.float32 and np.array_equal(tc.ordered_key(f), keys)
    assert int(np.isnan(f).sum()) == 63                      # NaNs of both signs, payloads kept by the round trip
    assert np.isposinf(f).any() and (f == 0).sum() == 1      # +inf = 0xFF800000, +0.0 = 0x80000000
    # the order of the bit image: -0.0 below +0.0, positive NaN above +inf, negative NaN below -inf
    z = np.array([0x00000000, 0x80000000, 0x7F800000, 0x7FC00000, 0xFF800000, 0xFFC00000], np.uint32).view(np.float32)
    kz = tc.ordered_key(z)
    assert kz[1] < kz[0] and kz[3] > kz[2] and kz[5] < kz[4]
    assert np.array_equal(tc.float_from_key(kz).view(np.uint32), z.view(np.uint32))
    edge = np.array([0, 1, 0x007FFFFF, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFF800000, 0xFFFFFFFF], np.uint32)
    assert np.array_equal(tc.ordered_key(tc.float_from_key(edge)), edge)


def test_sweep_reaches_every_digit_edge():
    """what the digit-edge sweep must contain, counted on the CPU"""
    uk, cnt, cum = tc.sweep_classes()
    ks = tc.sweep_ks()
    assert uk.shape[0] == 256 and cum[-1] == tc.SWEEP_ROWS
    assert len(tc.sweep_calls()) * tc.SWEEP_FRAMES >= len(ks) > 700
    sel = [k for k in ks if 0 < k < tc.SWEEP_ROWS]           # the frames that run the select
    thr = np.array([tc.sweep_threshold(k) for k in sel], dtype=np.uint32)
    for p in range(4):
        digit = (thr >> np.uint32(24 - 8 * p)) & np.uint32(0xFF)
        # digit 0x00: no digit >= 1 reaches k_rem in this pass; 0xFF: the walk stops at its first digit
        assert int((digit == 0x00).sum()) >= 150 and int((digit == 0xFF).sum()) >= 150, p
    above = np.concatenate([[0], cum[:-1]])
    assert any(int(a) + 1 in sel for a in above) and any(int(a + c) in sel and c > 1 for a, c in zip(above, cnt))
    assert 0 in ks and tc.SWEEP_ROWS in ks and tc.SWEEP_ROWS + 1 in ks   # keep none, keep all, k beyond the frame


def test_special_frames_hold_their_values():
    for name in tc.SPECIAL:
        lg, offs, k, thr = tc.special(name)
        for f, want in enumerate(thr):
            if want is not None:
                assert tc.threshold_key(lg, offs, k, f) == want, (name, f)
    lg, offs, k, _ = tc.special("neg_inf_mask")
    assert k[0] > int(np.isfinite(lg[:offs[1]]).sum())
    lg, offs, k, _ = tc.special("pos_inf")
    assert k[0] < int(np.isposinf(lg[:offs[1]]).sum())
    lg, offs, k, _ = tc.special("plus_zero")
    bits = lg.view(np.uint32)
    assert (bits[:offs[1]] == 0x80000000).sum() == 800 and (bits[:offs[1]] == 0).sum() == 800
    ref = tc.topk_ref(lg, offs, k)
    assert not (bits[ref[ref < offs[1]]] == 0x80000000).any()          # no -0.0 row survives next to a +0.0 threshold
    assert (bits[ref[ref >= offs[1]]] == 0).sum() == 800               # frame 1 keeps every +0.0 and some -0.0
    lg, offs, k, _ = tc.special("denormals")
    b = lg.view(np.uint32) & np.uint32(0x7FFFFFFF)
    assert b.max() < 64 and (lg.view(np.uint32) >> 31).any() and (b == 0).any() and (b > 0).any()
    lg, offs, k, _ = tc.special("nans")
    assert tc.threshold_key(lg, offs, k, 0) > 0xFF800000 and tc.threshold_key(lg, offs, k, 1) < 0x007FFFFF
    keys = tc.ordered_key(lg)
    assert np.unique(keys[keys > 0xFF800000]).shape[0] == len(tc.POS_NANS)
    assert np.unique(keys[keys < 0x007FFFFF]).shape[0] == len(tc.NEG_NANS)
    lg, offs, k, _ = tc.special("dense_last_byte")
    keys = tc.ordered_key(lg)
    assert np.unique(keys >> np.uint32(8)).shape[0] == 1 and np.unique(keys & np.uint32(0xFF)).shape[0] == 256
    lg, offs, k, _ = tc.special("top_byte_only")
    keys = tc.ordered_key(lg)
    assert np.unique(keys & np.uint32(0xFFFFFF)).shape[0] == 1 and np.unique(keys >> np.uint32(24)).shape[0] == 256


def test_placement_cases_select_their_form():
    for name in tc.TINY:
        lg, offs, k, four = tc.tiny(name)
        assert tc.four_launches(np.diff(offs)) == four, name
        assert lg.shape[0] == offs[-1]
    ks = [a for name in tc.TINY for a in tc.tiny(name)[2]]
    cs = [c for name in tc.TINY for c in np.diff(tc.tiny(name)[1])]
    assert 0 in ks and 1 in ks and any(a == c and c > 1 for a, c in zip(ks, cs))
    assert sum(np.diff(tc.tiny("12_frames_7_rows")[1])) == 7 and tc.staged(np.diff(tc.tiny("12_frames_7_rows")[1]))
    assert sum(np.diff(tc.tiny("120_frames_100_rows")[1])) == 100 and len(tc.tiny("120_frames_100_rows")[2]) == 120
    assert not tc.four_launches([2048 * 2048, 300]) and tc.four_launches([2048 * 2048 + 1, 300])
    lg, offs, k = tc.many_frames()
    assert len(k) == 120 and 0 in np.diff(offs) and not tc.four_launches(np.diff(offs))
    assert not tc.staged([1] * 8) and tc.staged([1] * 9)
    assert not tc.four_launches(tc.SEQ8) and tc.four_launches([1, 0, 0, 2])


def test_oracle_topk_equals_the_restatement(oracle):
    """oracle.topk (a qsort in C) and the numpy lexsort agree on every input set of topk_cases, NaN, +-inf and +-0
    among them"""
    for name, lg, offs, k in tc.all_inputs():
        ref = reference(oracle, name, lg, offs, k)
        assert np.array_equal(ref, tc.topk_ref(lg, offs, k)), name


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_digit_edge_sweep(rt, oracle):
    """every class boundary of 3000 rows over the byte alphabet, 8 frames (one k each) per call"""
    d = dev(rt, tc.sweep_calls()[0][0])                      # every call reads the same logits
    for i, (lg, offs, k) in enumerate(tc.sweep_calls()):
        ref = reference(oracle, "sweep%d" % i, lg, offs, k)
        keep, remap = rt.topk_prune(d, offs, k, with_map=True)
        assert np.array_equal(host(keep).view(np.uint32), ref), k
        assert np.array_equal(host(remap), tc.remap_ref(lg.shape[0], ref)), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.SPECIAL)
def test_special_values(rt, oracle, name):
    lg, offs, k, _ = tc.special(name)
    hold(rt, reference(oracle, name, lg, offs, k), lg, offs, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.TINY)
def test_tiny_frames_in_either_form(rt, oracle, name):
    lg, offs, k, four = tc.tiny(name)
    assert tc.four_launches(np.diff(offs)) == four
    hold(rt, reference(oracle, name, lg, offs, k), lg, offs, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tc.LARGE))
def test_frame_at_the_tile_limit(rt, oracle, name):
    """4 194 304 rows: the last frame two launches place; 4 194 305: flags, a three-launch scan, an emit whose grid strides"""
    lg, offs, k, four = tc.large(name)
    assert tc.four_launches(np.diff(offs)) == four
    hold(rt, reference(oracle, name, lg, offs, k), lg, offs, k, plain=False)


@pytest.mark.gpu
def test_eight_and_nine_frames(rt, oracle):
    """parameters as kernel arguments (8) and through staging (9): the oracle's rows, and frame for frame each other's"""
    lg, offs, k = tc.nine_frames()
    ref9 = reference(oracle, "nine_frames", lg, offs, k)
    ref8 = reference(oracle, "eight_frames", lg[:offs[8]], offs[:9], k[:8])
    hold(rt, ref9, lg, offs, k)
    hold(rt, ref8, lg[:offs[8]], offs[:9], k[:8])
    k9, m9 = rt.topk_prune(dev(rt, lg), offs, k, with_map=True)
    k8, m8 = rt.topk_prune(dev(rt, lg[:offs[8]]), offs[:9], k[:8], with_map=True)
    assert np.array_equal(host(k9)[:k8.shape[0]], host(k8)) and np.array_equal(host(m9)[:offs[8]], host(m8))


@pytest.mark.gpu
def test_120_frames(rt, oracle):
    lg, offs, k = tc.many_frames()
    hold(rt, reference(oracle, "many_frames", lg, offs, k), lg, offs, k)


@pytest.mark.gpu
def test_k_beyond_the_frame(rt, oracle):
    """k[f] > count[f] reaches the call unclamped: all rows of the frame, n_keep = sum of min(k, count)"""
    lg, offs, k = tc.oversized_k()
    assert max(k) == 2 ** 40 and k[0] == offs[1] + 1
    ref = reference(oracle, "oversized_k", lg, offs, k)
    hold(rt, ref, lg, offs, k)
    for f in (0, 1, 3):
        assert np.array_equal(ref[(ref >= offs[f]) & (ref < offs[f + 1])], np.arange(offs[f], offs[f + 1]))


@pytest.mark.gpu
def test_call_sequence_on_one_runtime(rt, oracle):
    """The histograms of calls of up to 8 frames live in two buffers of the context used in turn, each cleared by the
    call before: full buffers twice over, a call that returns before the flip (n == 0), a staged call and a four-launch
    call in between, and a call in which no frame selects, each against the oracle."""
    for step, counts in enumerate(tc.SEQUENCE):
        lg, offs, k = tc.sequence_call(step)
        if counts is None:
            keep, remap = rt.topk_prune(dev(rt, lg), offs, k, with_map=True)
            assert keep.shape[0] == 0 and remap.shape[0] == 0
            continue
        if step == tc.SEQ_NO_SELECT:
            assert all(a == 0 or a >= c for a, c in zip(k, counts))
        ref = reference(oracle, "sequence%d" % step, lg, offs, k)
        keep, remap = rt.topk_prune(dev(rt, lg), offs, k, with_map=True)
        assert np.array_equal(host(keep).view(np.uint32), ref), step
        assert np.array_equal(host(remap), tc.remap_ref(lg.shape[0], ref)), step


REFUSALS = {
    "no_frames": lambda lg, offs, k: (lg, [0], []),
    "121_frames": lambda lg, offs, k: (lg, [0] * 121 + [offs[-1]], [1] * 121),
    "first_offset": lambda lg, offs, k: (lg, [1] + offs[1:], k),
    "last_offset": lambda lg, offs, k: (lg, offs[:-1] + [offs[-1] - 1], k),
    "decreasing_offset": lambda lg, offs, k: (lg, offs[:2] + [offs[1] - 5] + offs[3:], k),
    "negative_k": lambda lg, offs, k: (lg, offs, k[:5] + [-1] + k[6:]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(rt, oracle, name):
    """PCC_E_ARG before any launch, and the next ordinary call of 8 frames is the oracle's"""
    PccError, E_ARG = pkg("runtime").PccError, pkg("_abi").PCC_E_ARG
    lg, offs, k = tc.sequence_call(0)
    bad = REFUSALS[name](lg, list(offs), list(k))
    for with_map in (False, True):
        with pytest.raises(PccError) as e:
            rt.topk_prune(dev(rt, bad[0]), bad[1], bad[2], with_map=with_map)
        assert e.value.code == E_ARG
    hold(rt, reference(oracle, "sequence0", lg, offs, k), lg, offs, k)
