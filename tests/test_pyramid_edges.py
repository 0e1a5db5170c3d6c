"""Stride-2 parents, the kernel-2 rule book and the pyramid sizes (csrc/pyramid.hip) at the seams of the tiled form
(8 keys of a thread, 512 of a wave, 2048 of a tile), beyond the first trip of the cross-tile sum, at the switch
between the two forms of pcc_down_coords_known, with a supplied count that is too small, and with batch bits in the
keys' top bits.  Inputs and the numpy reference: tests/map_cases.py.  Every comparison is equality of integers."""
import numpy as np
import pytest

import map_cases as mc
from conftest import pkg

U = np.uint64
SEAM_N = [1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097, 6145]
SEAM_CASES = [(n, p, cs) for n in SEAM_N for p in (("cycle", "singles") if n <= 9 else mc.PATTERNS) for cs in (0, 3)]
TILE_N = [526_336, 526_337, 528_385]                 # 257, 258, 259 tiles: the 256-strided sum starts a second trip
SWITCH_N = [4_194_304, 4_194_305]                    # the last size of the two-launch form, the first of flags-and-scan
BIG_CASES = [(n, p) for n in TILE_N + SWITCH_N for p in ("cycle7", "eights+3")]
BATCHES4 = (0, 1, 32768, 65534)
BATCHES17 = tuple(2 ** k - 1 for k in range(16)) + (65534,)     # neighbours differ first in bit 48, 49, ..., 63
SHIFT_CASES = [("cycle7", 12, 1, 3000), ("random", 12, 1, 3000), ("cycle7", 42, 1, 3000), ("random", 42, 1, 3000),
               ("cycle7", 0, (0, 1, 2), 3000), ("random", 12, (0, 1, 2), 3000), ("cycle7", 0, BATCHES4, 3000),
               ("random", 3, BATCHES4, 3000), ("singles", 0, BATCHES4, 4), ("singles", 12, BATCHES17, 17)]
COUNT_N = [1, 2, 2048, 2049, 524_288, 524_289, 4_194_304, 4_194_305, 4_196_353]
UP_CASES = [(n, cs) for n in (1, 31, 32, 33) for cs in (0, 6, 45)]
CANARY = 0x5A5A5A5A


def dev(rt, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return rt.to_device(a if a.flags.writeable else a.copy())


def host(t):
    return t.cpu().numpy()


def big_ref(oracle, keys, cshift):
    """(pkeys, nbr8, parent_of) of a large set: oracle.down, and parent_of as the running count of parent changes"""
    rpk, rnbr8 = oracle.down(keys, 1 << (cshift // 3))
    pk = keys >> U(cshift + 3)
    po = np.concatenate([[0], np.cumsum(pk[1:] != pk[:-1])]).astype(np.int32)
    return rpk, rnbr8, po


def last_pair_cases(n):
    """a "random" key set whose last pair is the only batch change / the only repeat"""
    keys = mc.parent_runs(n, "random", 0)[0]
    assert int(keys[-1] >> U(48)) == 0
    if n < 2:
        return {"plain": keys.copy()}
    a, b = keys.copy(), keys.copy()
    a[-1] |= U(1 << 48)
    b[-1] = b[-2]
    return {"batch_change": a, "repeat": b}


def seams_wanted(n, pattern):
    """which seams a pattern must have a parent across, from its construction"""
    if pattern in ("singles", "eights"):
        return (False, False, False)
    if pattern == "random":
        return (n >= 511, False, False)
    return (n >= 9, n >= 513, n >= 2049)


# ------------------------------------------------------------------ the reference and the inputs (no GPU)
@pytest.mark.parametrize("n", SEAM_N)
def test_down_ref_equals_oracle_on_the_seam_sets(oracle, n):
    for nn, pattern, cshift in SEAM_CASES:
        if nn != n:
            continue
        keys, seams = mc.parent_runs(n, pattern, cshift)
        assert keys.shape[0] == n and np.all(keys & U((1 << cshift) - 1) == 0)
        for have, want in zip(seams, seams_wanted(n, pattern)):
            assert have > 0 or not want, (n, pattern, seams)
        if pattern == "eights":
            assert seams == (0, 0, 0)                         # a thread's eight keys are one parent
        rpk, rnbr8, rpo = mc.down_ref(keys, cshift)
        opk, onbr8 = oracle.down(keys, 1 << (cshift // 3))
        assert np.array_equal(rpk, opk) and np.array_equal(rnbr8, onbr8)
        assert np.array_equal(rpk[rpo], (keys >> U(cshift + 3)) << U(cshift + 3))
        if pattern == "singles":
            assert rpk.shape[0] == n
        counts, dup = mc.level_counts_ref(keys, cshift, 4)
        cur, s = keys, 1 << (cshift // 3)
        for lvl in range(4):
            cur, s = oracle.down(cur, s)[0], 2 * s
            assert counts[lvl] == cur.shape[0]
        assert not dup


@pytest.mark.parametrize("n,pattern", BIG_CASES)
def test_down_ref_equals_oracle_on_the_large_sets(oracle, n, pattern):
    keys, seams = mc.parent_runs(n, pattern, 0)
    assert keys.shape[0] == n and min(seams) > 0
    assert (n + 2047) // 2048 in (257, 258, 259, 2048, 2049)
    rpk, rnbr8, rpo = mc.down_ref(keys, 0)
    opk, onbr8, opo = big_ref(oracle, keys, 0)
    assert np.array_equal(rpk, opk) and np.array_equal(rnbr8, onbr8) and np.array_equal(rpo, opo)


@pytest.mark.parametrize("pattern,cshift,batches,n", SHIFT_CASES)
def test_refs_equal_oracle_with_other_shifts_and_batches(oracle, pattern, cshift, batches, n):
    keys, _ = mc.parent_runs(n, pattern, cshift, batches)
    if batches != 1:
        per = n // len(batches)
        low = keys & U((1 << 48) - 1)
        assert np.array_equal(low[:per], low[per:2 * per]) and len(set(int(v) for v in keys >> U(48))) == len(batches)
    if n <= 17:                                               # one key per batch: neighbours have the same low 48 bits
        assert np.unique(keys & U((1 << 48) - 1)).shape[0] == 1
    rpk, rnbr8, rpo = mc.down_ref(keys, cshift)
    opk, onbr8 = oracle.down(keys, 1 << (cshift // 3))
    assert np.array_equal(rpk, opk) and np.array_equal(rnbr8, onbr8)
    if batches != 1:
        assert rpk.shape[0] == len(batches) * mc.down_ref(keys[:n // len(batches)], cshift)[0].shape[0]


def test_level_counts_ref_equals_successive_oracle_down(oracle):
    sets = {"b4": (mc.parent_runs(5000, "random", 0, BATCHES4)[0], 0, 16),
            "b17": (mc.parent_runs(5100, "random", 0, BATCHES17)[0], 0, 16),
            "shift9": (mc.parent_runs(5000, "random", 9, BATCHES4)[0], 9, 13)}
    assert mc.diff_bits(sets["b4"][0]) >= {48, 62, 63}
    assert mc.diff_bits(sets["b17"][0]) >= set(range(48, 64))
    for n in COUNT_N:
        if n <= 600_000:
            for what, keys in last_pair_cases(n).items():
                sets["%s_%d" % (what, n)] = (keys, 0, 3)
    for name, (keys, cshift, levels) in sets.items():
        counts, dup = mc.level_counts_ref(keys, cshift, levels)
        assert dup == name.startswith("repeat"), name
        cur, s = np.unique(keys), 1 << (cshift // 3)
        for lvl in range(levels):
            cur, s = oracle.down(cur, s)[0], 2 * s
            assert counts[lvl] == cur.shape[0], (name, lvl)
    assert mc.level_counts_ref(sets["b17"][0], 0, 16)[0][-1] == 17       # at shift 48 the batches are left


@pytest.mark.parametrize("n", COUNT_N)
def test_last_pair_cases_are_what_they_say(n):
    for what, keys in last_pair_cases(n).items():
        d = keys[1:] ^ keys[:-1]
        if what == "batch_change":
            assert np.all(d[:-1] < U(1 << 48)) and d[-1] >= U(1 << 48) and np.all(d != 0)
        if what == "repeat":
            assert np.all(d[:-1] != 0) and d[-1] == 0


# ------------------------------------------------------------------ GPU: pcc_down_coords / _known
def three_way(rt, keys, cshift, ref):
    """pcc_down_coords, pcc_down_coords_known with the count of pcc_level_counts, and the reference"""
    rpk, rnbr8, rpo = ref
    m = rpk.shape[0]
    kd = dev(rt, keys)
    assert rt.level_counts(kd, cshift, 1) == ([m], False)
    for m_known in (None, m):
        pk, nbr8, po = rt.down_coords(kd, cshift, m_known=m_known)
        assert pk.shape[0] == m, m_known
        assert np.array_equal(host(pk).view(U), rpk), m_known
        assert np.array_equal(host(nbr8), rnbr8), m_known
        assert np.array_equal(host(po), rpo), m_known


@pytest.mark.gpu
@pytest.mark.parametrize("n,pattern,cshift", SEAM_CASES)
def test_seams(rt, n, pattern, cshift):
    """a parent's children on both sides of a thread's 8 keys, a wave's 512 and a tile's 2048; keys[base - 1] as the
    predecessor of a thread's first key"""
    keys, seams = mc.parent_runs(n, pattern, cshift)
    for have, want in zip(seams, seams_wanted(n, pattern)):
        assert have > 0 or not want
    three_way(rt, keys, cshift, mc.down_ref(keys, cshift))


@pytest.mark.gpu
@pytest.mark.parametrize("n,pattern", BIG_CASES)
def test_cross_tile_sum_and_route_switch(rt, oracle, n, pattern):
    keys, seams = mc.parent_runs(n, pattern, 0)
    assert min(seams) > 0
    three_way(rt, keys, 0, big_ref(oracle, keys, 0) if n in SWITCH_N else mc.down_ref(keys, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,cshift,batches,n", SHIFT_CASES)
def test_other_shifts_and_batches(rt, pattern, cshift, batches, n):
    """the batch index is part of the parent: equal low 48 bits in neighbouring batches are different parents"""
    keys, _ = mc.parent_runs(n, pattern, cshift, batches)
    three_way(rt, keys, cshift, mc.down_ref(keys, cshift))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2049, 4_194_305])
def test_a_supplied_count_that_is_too_small(rt, oracle, n):
    """m below the real parent count: the first m parents complete, nothing written beyond them.  The buffers are as
    large as the real count needs, whatever the guard does."""
    rtm = pkg("runtime")
    torch = pytest.importorskip("torch")
    keys, _ = mc.parent_runs(n, "cycle7", 0)
    rpk, rnbr8, rpo = big_ref(oracle, keys, 0)
    m_true = rpk.shape[0]
    kd = dev(rt, keys)
    for m in (m_true - 1, 1):
        pk = torch.full((n,), CANARY, dtype=torch.int64, device=rt.device)
        nbr8 = torch.full((8 * n,), CANARY, dtype=torch.int32, device=rt.device)
        po = torch.full((n,), CANARY, dtype=torch.int32, device=rt.device)
        rtm.check(rt.lib.pcc_down_coords_known(rt.ctx, rtm._ptr(kd), n, 0, rtm._ptr(pk), rtm._ptr(nbr8), n, rtm._ptr(po), m),
                  "pcc_down_coords_known")
        pk, nbr8, po = host(pk), host(nbr8), host(po)
        assert np.array_equal(pk[:m].view(U), rpk[:m]), m
        assert np.array_equal(nbr8[:8 * m].reshape(8, m), rnbr8[:, :m]), m
        assert np.array_equal(po, np.where(rpo < m, rpo, CANARY)), m
        assert np.all(pk[m:] == CANARY) and np.all(nbr8[8 * m:] == CANARY), m


# ------------------------------------------------------------------ GPU: pcc_level_counts
@pytest.mark.gpu
def test_level_counts_with_batch_bits(rt):
    """bins 48 ... 63 of the histogram: neighbours in different batches, bit 63 with a batch index >= 32768"""
    for keys, cshift, levels, bins in ((mc.parent_runs(5000, "random", 0, BATCHES4)[0], 0, 16, {48, 62, 63}),
                                       (mc.parent_runs(5100, "random", 0, BATCHES17)[0], 0, 16, set(range(48, 64))),
                                       (mc.parent_runs(5000, "random", 9, BATCHES4)[0], 9, 13, {48, 62, 63})):
        assert mc.diff_bits(keys) >= bins
        assert rt.level_counts(dev(rt, keys), cshift, levels) == mc.level_counts_ref(keys, cshift, levels)


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNT_N)
def test_level_counts_last_pair(rt, n):
    """the grid is capped at 2048 workgroups of 2048 keys; the last pair is the last trip of the last thread"""
    for what, keys in last_pair_cases(n).items():
        ref = mc.level_counts_ref(keys, 0, 3)
        assert ref[1] == (what == "repeat")
        assert rt.level_counts(dev(rt, keys), 0, 3) == ref, what


# ------------------------------------------------------------------ GPU: pcc_up_coords / _rows
@pytest.mark.gpu
@pytest.mark.parametrize("n,cshift", UP_CASES)
def test_up_coords(rt, oracle, n, cshift):
    keys, _ = mc.parent_runs(n, "singles", cshift + 3)
    ref = oracle.up(keys, 2 << (cshift // 3))
    assert np.array_equal(ref, mc.up_keys(keys, cshift)) and np.all(ref[1:] > ref[:-1])
    kd = dev(rt, keys)
    assert np.array_equal(host(rt.up_coords(kd, cshift)).view(U), ref)
    for rows in (np.arange(0), np.arange(8 * n), np.arange(8 * n)[::-1]):
        r = rows.astype(np.uint32)
        want = keys[r >> 3] | ((r & 7).astype(U) << U(cshift))
        got = host(rt.up_coords_rows(kd, cshift, dev(rt, r))).view(U)
        assert got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------ GPU: refusals
@pytest.mark.gpu
def test_refusals_leave_the_runtime_usable(rt):
    abi = pkg("_abi")
    keys, _ = mc.parent_runs(2049, "cycle7", 0)
    ref = mc.down_ref(keys, 0)
    kd = dev(rt, keys)
    n = keys.shape[0]
    bad = [lambda: rt.level_counts(kd, 0, 0), lambda: rt.level_counts(kd, 0, 17), lambda: rt.level_counts(kd, 1, 3),
           lambda: rt.level_counts(kd, 36, 5), lambda: rt.down_coords(kd, 2), lambda: rt.down_coords(kd, 45),
           lambda: rt.down_coords(kd, 0, m_known=0), lambda: rt.down_coords(kd, 0, m_known=n + 1)]
    for i, call in enumerate(bad):
        with pytest.raises(abi.PccError) as e:
            call()
        assert e.value.code == abi.PCC_E_ARG, i
        assert rt.level_counts(kd, 0, 2) == mc.level_counts_ref(keys, 0, 2), i
        pk, nbr8, po = rt.down_coords(kd, 0, m_known=ref[0].shape[0])
        assert np.array_equal(host(pk).view(U), ref[0]) and np.array_equal(host(nbr8), ref[1]), i
