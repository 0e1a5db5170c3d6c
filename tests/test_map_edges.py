"""Coordinate maps (csrc/map.hip) and the key helpers of csrc/sort.hip at the sizes where pcc_build_map changes its
route, at the faces of the coordinate cube in every route, on probe chains made by inverting hash64, and at the edges of
the derived books.  Inputs and the numpy reference: tests/map_cases.py.  Every comparison is equality of integers."""
import ctypes as C
import functools

import numpy as np
import pytest

import map_cases as mc
from conftest import pkg

U = np.uint64
ROUTE_N = [1, 2, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 70_001]
WRAP_STRIDES = [1, 2, 8, 16384]
WRAP_N = [0, 5000, 66_000]                       # 0: the wrap rows alone (LDS route); hash route; batched route
CHAIN_N = [5000, 66_000]
CHAIN_CAP = {5000: 32768, 66_000: 524_288}
UP_N = [1, 31, 32, 33, 1000]
DOWN_N = [1, 255, 256, 257, 5000]


def dev(rt, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return rt.to_device(a if a.flags.writeable else a.copy())


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------ the input sets, each built once
def _seed(name):
    return np.random.default_rng([ord(ch) for ch in name])


def _edge_cluster():
    """27 rows around (32766, 32766, 32766) in batches 0 and 65534: the last is key 0xFFFE_FFFF_FFFF_FFFF"""
    g = np.array([(x, y, z) for x in (32765, 32766, 32767) for y in (32765, 32766, 32767) for z in (32765, 32766, 32767)])
    return np.concatenate([np.concatenate([np.full((27, 1), b), g], 1) for b in (0, 65534)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def map_set(name):
    """name -> (sorted distinct keys, stride, extras)"""
    kind, *arg = name.split(":")
    rng = _seed(name)
    if kind == "route":
        n, stride = int(arg[0]), int(arg[1])
        return mc.sorted_keys(mc.lattice_cloud(rng, n, stride, batches=2)), stride, {}
    if kind == "wrap":
        stride, n = int(arg[0]), int(arg[1])
        rows, _ = mc.wrap_rows(stride)
        keys = mc.sorted_keys(rows)
        if n:
            if stride == 16384:                  # four lattice points per axis: 64 per batch, half of them taken
                nb = -(-2 * n // 64)
                keys = mc.pad_keys(rng, keys, n, stride, batches=nb, box=64 * nb)
            else:
                keys = mc.pad_keys(rng, keys, n, stride, batches=2)
        return keys, stride, {"wrap": mc.wrap_entries(keys, stride)}
    if kind == "marker":
        n = int(arg[0])
        return mc.pad_keys(rng, mc.coords_keys(_edge_cluster()), n, 1, batches=2, batch_ids=(0, 65534)), 1, {}
    if kind == "chain":
        n = int(arg[0])
        cap = CHAIN_CAP[n]
        chains, wit, absent = [], [], []
        for slot in (cap // 2, cap - 3):
            ck, w = mc.collision_chain(cap, slot, 48, rng)
            chains.append(ck)
            wit.append(w)
            absent.append(mc.collision_chain(cap, slot, 30, rng)[0])
        chains, wit = np.concatenate(chains), np.concatenate(wit)
        keys = mc.pad_keys(rng, np.concatenate([chains, wit]), n, 1, batches=2)
        absent = np.concatenate([a[~np.isin(a, keys)][:24] for a in absent])
        return keys, 1, {"chains": chains, "witnesses": wit, "absent": absent, "cap": cap}
    if kind == "par":                            # a parent level at stride 2
        n = int(arg[0])
        return mc.sorted_keys(mc.lattice_cloud(rng, n, 2, batches=2, box=None if n > 100 else 2 * n)), 2, {}
    if kind == "up":                             # its 8 n generative children at stride 1
        return mc.up_keys(map_set("par:" + arg[0])[0], 0), 1, {}
    if kind == "down":
        n = int(arg[0])
        return mc.sorted_keys(mc.lattice_cloud(rng, n, 1, batches=2)), 1, {}
    raise KeyError(name)


MAP_SETS = (["route:%d:%d" % (n, s) for n in ROUTE_N for s in (1, 8)] +
            ["wrap:%d:%d" % (s, n) for s in WRAP_STRIDES for n in WRAP_N] +
            ["marker:%d" % n for n in CHAIN_N] + ["chain:%d" % n for n in CHAIN_N] +
            ["par:%d" % n for n in UP_N] + ["up:%d" % n for n in UP_N] + ["down:%d" % n for n in DOWN_N])
# the sets drawn by lattice_cloud with enough rows for a share: a book of n rows has at most (n - 1) / 26 hits per
# entry, so n = 1 and n = 2 cannot reach 20 %
SHARED = [s for s in MAP_SETS if s.split(":")[0] in ("route", "par", "down", "marker", "chain") and
          int(s.split(":")[1]) > 2] + ["wrap:%d:%d" % (s, n) for s in WRAP_STRIDES for n in WRAP_N[1:]]


@functools.lru_cache(maxsize=None)
def ref27(name):
    keys, stride, _ = map_set(name)
    return mc.map27_ref(keys, stride)


def assert_share(name):
    """neither branch of a probe is rare: 20 % to 60 % of the non-centre entries of the reference book are rows"""
    share = mc.hit_share(ref27(name))
    assert 0.20 <= share <= 0.60, (name, share)


# ------------------------------------------------------------------ the reference and the inputs (no GPU)
def test_restatements(oracle):
    rng = np.random.default_rng(1)
    c = np.concatenate([rng.integers(0, 65535, (4000, 1)), rng.integers(-32768, 32768, (4000, 3))], 1).astype(np.int32)
    c[:4] = [[0, -32768, -32768, -32768], [65534, 32767, 32767, 32767], [0, 32767, -32768, 0], [65534, 0, 0, -1]]
    keys = mc.coords_keys(c)
    assert np.array_equal(keys, oracle.morton_keys(c))
    assert int(keys[1]) == 0xFFFE_FFFF_FFFF_FFFF
    assert np.array_equal(np.stack(mc.unmorton(keys), 1), c)
    k = np.concatenate([rng.integers(0, 1 << 64, 100_000, dtype=np.uint64), np.array([0, 1, 2 ** 64 - 2], dtype=U)])
    assert np.array_equal(mc.hash64_inv(mc.hash64(k)), k) and np.array_equal(mc.hash64(mc.hash64_inv(k)), k)
    assert int(mc.hash64(np.array([0], dtype=U))[0]) == 0 and mc.C1 * mc.C1_INV % 2 ** 64 == 1 == mc.C2 * mc.C2_INV % 2 ** 64
    # murmur3's finaliser on 1, worked with Python integers
    h = 1
    for mul in (mc.C1, mc.C2):
        h = ((h ^ (h >> 33)) * mul) % 2 ** 64
    assert int(mc.hash64(np.array([1], dtype=U))[0]) == h ^ (h >> 33)
    assert [mc.hash_capacity(n) for n in (0, 1, 256, 257, 4097, 5000, 8192, 8193, 65536, 65537, 66_000, 70_001)] == \
        [1024, 1024, 1024, 2048, 32768, 32768, 32768, 65536, 262_144, 524_288, 524_288, 524_288]
    for n in CHAIN_N:
        assert mc.hash_capacity(n) == CHAIN_CAP[n]


@pytest.mark.parametrize("name", MAP_SETS)
def test_map27_ref_equals_oracle(oracle, name):
    keys, stride, _ = map_set(name)
    assert np.all(keys[1:] > keys[:-1])
    want = {"route": 1, "wrap": 2, "marker": 1, "chain": 1, "par": 1, "up": 1, "down": 1}[name.split(":")[0]]
    n = int(name.split(":")[want])
    assert keys.shape[0] == (n or 21) * (8 if name.startswith("up") else 1)
    assert np.array_equal(ref27(name), oracle.map27(keys, stride))
    if name in SHARED:
        assert_share(name)


@pytest.mark.parametrize("stride", WRAP_STRIDES)
def test_wrap_rows_name_entries_on_every_axis(stride):
    rows, per_axis = mc.wrap_rows(stride)
    assert rows.shape[0] == 21 and np.all(rows[:, 1:] % stride == 0)
    for ax in range(3):
        assert per_axis[ax].shape[0] > 0, (stride, ax)
    for n in WRAP_N:
        keys, _, ex = map_set("wrap:%d:%d" % (stride, n))
        b, x, y, z = mc.unmorton(keys)
        assert np.all(x % stride == 0) and np.all(y % stride == 0) and np.all(z % stride == 0)
        for ax in range(3):
            e = ex["wrap"][ax]
            assert e.shape[0] >= per_axis[ax].shape[0] and np.all(ref27("wrap:%d:%d" % (stride, n))[e[:, 0], e[:, 1]] == -1)


@pytest.mark.parametrize("n", CHAIN_N)
def test_chains_sit_on_their_home_slots(n):
    keys, _, ex = map_set("chain:%d" % n)
    cap = ex["cap"]
    assert mc.hash_capacity(n) == cap and keys.shape[0] == n
    home = mc.hash64(ex["chains"]) & U(cap - 1)
    assert np.array_equal(np.unique(home, return_counts=True)[1], [48, 48])
    assert set(int(h) for h in home) == {cap // 2, cap - 3} and cap - 3 + 48 > cap        # the second runs over the end
    assert np.unique(ex["chains"]).shape[0] == 96 and not np.any(ex["chains"] == U(mc.HASH_EMPTY))
    assert np.all(np.isin(ex["chains"], keys)) and np.all(np.isin(ex["witnesses"], keys))
    assert ex["absent"].shape[0] == 48 and not np.any(np.isin(ex["absent"], keys))
    assert set(int(h) for h in mc.hash64(ex["absent"]) & U(cap - 1)) == {cap // 2, cap - 3}
    assert ex["witnesses"].shape[0] >= 90
    w = np.searchsorted(keys, ex["witnesses"])
    b, x, y, z = mc.unmorton(ex["witnesses"])
    assert np.array_equal(keys[ref27("chain:%d" % n)[4, w]], mc.morton(b, x - 1, y, z))   # offset 4 = (-1, 0, 0)
    assert np.all(np.isin(mc.morton(b, x - 1, y, z), ex["chains"]))


def test_marker_sets_hold_the_last_key():
    for n in CHAIN_N:
        keys, _, _ = map_set("marker:%d" % n)
        assert int(keys[-1]) == 0xFFFE_FFFF_FFFF_FFFF and keys.shape[0] == n
        b = mc.unmorton(keys)[0]
        assert set(int(v) for v in np.unique(b)) == {0, 65534}
        assert np.all(np.isin(mc.coords_keys(_edge_cluster()), keys))


# ------------------------------------------------------------------ GPU: pcc_build_map
@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 8])
@pytest.mark.parametrize("n", ROUTE_N)
def test_route_switches(rt, n, stride):
    """LDS search up to 4096 rows, one thread per (row, offset) up to 65536, batched probe rounds above; 70 001 rows
    end in a workgroup of one full wave, one partial wave and two idle ones"""
    name = "route:%d:%d" % (n, stride)
    keys, _, _ = map_set(name)
    if name in SHARED:
        assert_share(name)
    nbr = host(rt.build_map(dev(rt, keys), stride))
    assert np.array_equal(nbr, ref27(name))


@pytest.mark.gpu
@pytest.mark.parametrize("n", WRAP_N)
@pytest.mark.parametrize("stride", WRAP_STRIDES)
def test_range_edges_in_every_route(rt, stride, n):
    """rows on opposite faces of the cube are neighbours mod 2^16 only; every route carries its own range check"""
    name = "wrap:%d:%d" % (stride, n)
    keys, _, ex = map_set(name)
    if n:
        assert_share(name)
    nbr = host(rt.build_map(dev(rt, keys), stride))
    for ax in range(3):
        e = ex["wrap"][ax]
        assert e.shape[0] > 0
        got = nbr[e[:, 0], e[:, 1]]
        assert np.all(got == -1), ("axis %d wraps" % ax, e[got != -1][:8].tolist())
    assert np.array_equal(nbr, ref27(name))


@pytest.mark.gpu
@pytest.mark.parametrize("n", CHAIN_N)
def test_keys_next_to_the_empty_marker(rt, n):
    name = "marker:%d" % n
    keys, _, _ = map_set(name)
    assert_share(name)
    kd = dev(rt, keys)
    assert np.array_equal(host(rt.build_map(kd, 1)), ref27(name))
    c = _edge_cluster()
    q = np.concatenate([mc.coords_keys(c), mc.coords_keys(c - np.array([1, 0, 0, 0])[None, :] * (c[:, :1] > 0)),
                        np.array([0xFFFE_FFFF_FFFF_FFFE, 0xFFFD_FFFF_FFFF_FFFF], dtype=U)])
    at = np.minimum(np.searchsorted(keys, q), n - 1)
    want = np.where(keys[at] == q, at, -1).astype(np.int32)
    assert (want[:54] >= 0).all() and (want >= 0).sum() >= 54 and (want < 0).sum() >= 2
    assert np.array_equal(host(rt.lookup(kd, dev(rt, q))), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", CHAIN_N)
def test_probe_chains(rt, n):
    """two chains of 48 keys on one home slot each (one runs over the table's end), their (-1, 0, 0) witnesses, and
    queries that walk a whole chain.  Which chain key sits at which depth is decided by atomics and is not assumed."""
    name = "chain:%d" % n
    keys, _, ex = map_set(name)
    assert mc.hash_capacity(n) == ex["cap"]
    assert_share(name)
    kd = dev(rt, keys)
    nbr = host(rt.build_map(kd, 1))
    w = np.searchsorted(keys, ex["witnesses"])
    b, x, y, z = mc.unmorton(ex["witnesses"])
    chain_row = np.searchsorted(keys, mc.morton(b, x - 1, y, z))
    assert np.array_equal(nbr[4, w], chain_row.astype(np.int32))
    assert np.array_equal(nbr, ref27(name))
    rng = np.random.default_rng(n)
    far = rng.integers(0, 65535 << 48, 1200, dtype=np.uint64)
    far = far[~np.isin(far, keys)][:1000]
    q = np.concatenate([ex["chains"], ex["absent"], keys[rng.integers(0, n, 1000)], far])
    at = np.minimum(np.searchsorted(keys, q), n - 1)
    want = np.where(keys[at] == q, at, -1).astype(np.int32)
    assert (want[:96] >= 0).all() and (want[96:144] == -1).all() and (want >= 0).sum() == 1096
    assert np.array_equal(host(rt.lookup(kd, dev(rt, q))), want)


@pytest.mark.gpu
def test_lookup_in_an_empty_key_set(rt):
    q = np.random.default_rng(3).integers(0, 65535 << 48, 300, dtype=np.uint64)
    rows = host(rt.lookup(dev(rt, np.zeros(0, dtype=U)), dev(rt, q)))
    assert rows.shape == (300,) and np.all(rows == -1)


# ------------------------------------------------------------------ GPU: derived books
def _keeps(n):
    return {"every_second": np.arange(0, n, 2), "row_0": np.array([0]), "last_row": np.array([n - 1]), "all": np.arange(n)}


@pytest.mark.gpu
@pytest.mark.parametrize("n_par", UP_N)
def test_derive_map_up(rt, n_par):
    """8 n_par children cross the 256-thread workgroup at n_par = 32"""
    pk, _, _ = map_set("par:%d" % n_par)
    if n_par > 2:
        assert_share("par:%d" % n_par)
    nbr_p = rt.build_map(dev(rt, pk), 2)
    assert np.array_equal(host(rt.derive_map_up(nbr_p, n_par)), ref27("up:%d" % n_par))
    for what, keep in _keeps(n_par).items():
        keep_d = dev(rt, keep.astype(np.uint32))
        remap = rt.inverse_rows(keep_d, n_par)
        nbr = host(rt.derive_map_up(nbr_p, len(keep), keep_d, remap))
        assert np.array_equal(nbr, mc.map27_ref(mc.up_keys(pk[keep], 0), 1)), what


@pytest.mark.gpu
@pytest.mark.parametrize("n_par", UP_N)
def test_subset_map_up(rt, n_par):
    pk, _, _ = map_set("par:%d" % n_par)
    nbr_p = rt.build_map(dev(rt, pk), 2)
    full = ref27("up:%d" % n_par)
    nc = 8 * n_par
    keeps = {"one_child": np.array([min(5, nc - 1)]), "last_parents_8": np.arange(nc - 8, nc),
             "every_third": np.arange(0, nc, 3), "all": np.arange(nc)}
    for what, keep in keeps.items():
        remap_ref = np.full(nc, -1, dtype=np.int32)
        remap_ref[keep] = np.arange(len(keep), dtype=np.int32)
        want = np.where(full[:, keep] >= 0, remap_ref[np.maximum(full[:, keep], 0)], -1).astype(np.int32)
        keep_d = dev(rt, keep.astype(np.uint32))
        remap = rt.inverse_rows(keep_d, nc)
        assert np.array_equal(host(remap), remap_ref), what
        assert np.array_equal(host(rt.subset_map_up(nbr_p, keep_d, remap)), want), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", DOWN_N)
def test_derive_map_down(rt, n):
    name = "down:%d" % n
    keys, _, _ = map_set(name)
    if n > 2:
        assert_share(name)
    kd = dev(rt, keys)
    pk, nbr8, parent_of = rt.down_coords(kd, 0)
    rpk, rnbr8, rpo = mc.down_ref(keys, 0)
    assert np.array_equal(host(pk).view(U), rpk) and np.array_equal(host(nbr8), rnbr8) and np.array_equal(host(parent_of), rpo)
    nbr_p = rt.build_map(pk, 2)
    assert np.array_equal(host(nbr_p), mc.map27_ref(rpk, 2))
    nbr = rt.derive_map_down(nbr_p, nbr8.contiguous(), parent_of, kd, 0)
    assert np.array_equal(host(nbr), ref27(name))


@pytest.mark.gpu
def test_inverse_rows_edges(rt):
    """m = n skips the preset (every entry must come from the rows), m = 0 is the preset alone"""
    rtm = pkg("runtime")
    n = 1000
    rng = np.random.default_rng(11)
    perm = rng.permutation(n).astype(np.uint32)
    for what, rows in (("m=0", perm[:0]), ("m=1", np.array([n - 1], dtype=np.uint32)), ("m=n", perm), ("m=n-1", perm[:-1])):
        remap = dev(rt, np.full(n, 7, dtype=np.int32))
        rtm.check(rt.lib.pcc_inverse_rows(rt.ctx, rtm._ptr(dev(rt, rows)), len(rows), n, rtm._ptr(remap)), "pcc_inverse_rows")
        want = np.full(n, -1, dtype=np.int32)
        want[rows.astype(np.int64)] = np.arange(len(rows), dtype=np.int32)
        assert np.array_equal(host(remap), want), what


@pytest.mark.gpu
def test_gather_map_columns_with_absent_rows(rt):
    keys, _, _ = map_set("par:1000")
    n = keys.shape[0]
    kd = dev(rt, keys)
    book27 = rt.build_map(kd, 2)
    _, book8, _ = rt.down_coords(kd, 3)
    rng = np.random.default_rng(12)
    for book in (book27, book8.contiguous()):
        hb = host(book)
        rows = rng.integers(0, hb.shape[1], 333).astype(np.int32)
        rows[::5] = -1
        rows[-1] = -1
        assert rows[0] == -1 and (rows >= 0).sum() > 200
        out, me = rt.gather_map_columns(book, dev(rt, rows))
        want = np.where(rows[None, :] >= 0, hb[:, np.maximum(rows, 0)], -1).astype(np.int32)
        assert np.array_equal(host(out), want)
        assert np.array_equal(host(me), np.where(rows >= 0, np.arange(333), -1).astype(np.int32))
    assert n == 1000


# ------------------------------------------------------------------ GPU: key helpers of sort.hip
@pytest.mark.gpu
def test_morton_keys_round_trip_on_the_corners(rt):
    c = np.array([(b, x, y, z) for b in (0, 65534) for x in (-32768, 32767) for y in (-32768, 32767)
                  for z in (-32768, 32767)], dtype=np.int32)
    assert c.shape == (16, 4)
    k = rt.morton_keys(dev(rt, c))
    assert np.array_equal(host(k).view(U), mc.coords_keys(c))
    assert np.array_equal(host(rt.keys_to_coords(k)), c)


@pytest.mark.gpu
@pytest.mark.parametrize("col,value", [(1, 32768), (1, -32769), (2, 32768), (2, -32769), (3, 32768), (3, -32769),
                                       (0, -1), (0, 65535)])
def test_morton_keys_refuses_the_first_value_outside(rt, col, value):
    """the offending row is the last of 257: the second workgroup raises the flag"""
    abi = pkg("_abi")
    c = mc.lattice_cloud(np.random.default_rng(13), 257, 1, batches=2)
    good = c.copy()
    good[-1, col] = {32768: 32767, -32769: -32768, -1: 0, 65535: 65534}[value]
    c[-1, col] = value
    with pytest.raises(abi.PccError) as e:
        rt.morton_keys(dev(rt, c))
    assert e.value.code == abi.PCC_E_RANGE
    assert np.array_equal(host(rt.morton_keys(dev(rt, good))).view(U), mc.coords_keys(good))


@pytest.mark.gpu
@pytest.mark.parametrize("n_batch", [1, 3, 63, 64, 65, 200])
def test_batch_offsets_with_empty_batches(rt, n_batch):
    rng = np.random.default_rng(n_batch)
    low = np.sort(rng.choice(1 << 20, 40, replace=False)).astype(U)
    used = {"all": range(n_batch), "empty_front_middle_end": [b for b in range(n_batch) if b % 3 == 1 and b < n_batch - 1],
            "last_only": [n_batch - 1], "none": []}
    for what, bs in used.items():
        keys = np.concatenate([np.zeros(0, dtype=U)] + [(U(b) << U(48)) | low for b in bs])
        want = [int(v) for v in np.searchsorted(keys, np.arange(n_batch + 1, dtype=U) << U(48))]
        assert rt.batch_offsets(dev(rt, keys), n_batch) == want, what
        assert want[-1] == keys.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 256, 257, 100_003])
def test_check_unique(rt, n):
    rtm = pkg("runtime")

    def dup(keys):
        flag = C.c_int(-5)
        rtm.check(rt.lib.pcc_check_unique(rt.ctx, rtm._ptr(dev(rt, keys)), len(keys), C.byref(flag)), "pcc_check_unique")
        return flag.value

    base = np.arange(n, dtype=U) * U(4) + U(8)
    assert dup(base) == 0
    bit0 = base.copy()
    bit0[1::2] = bit0[0:n - 1:2] + U(1)                     # neighbours that differ in bit 0 only
    assert n < 2 or np.all((bit0[1::2] ^ bit0[0:n - 1:2]) == U(1))
    assert dup(bit0) == 0
    for i in (0, 255, n - 2):
        if 0 <= i and i + 1 < n:
            k = base.copy()
            k[i + 1] = k[i]
            assert dup(k) != 0, (i, i + 1)
            assert dup(base) == 0


# ------------------------------------------------------------------ GPU: refusals
@pytest.mark.gpu
@pytest.mark.parametrize("stride", [0, 3, 32768])
def test_build_map_refuses_a_stride(rt, stride):
    abi = pkg("_abi")
    keys, _, _ = map_set("route:257:1")
    kd = dev(rt, keys)
    with pytest.raises(abi.PccError) as e:
        rt.build_map(kd, stride)
    assert e.value.code == abi.PCC_E_ARG
    assert np.array_equal(host(rt.build_map(kd, 1)), ref27("route:257:1"))
