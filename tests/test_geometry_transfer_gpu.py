"""GeometryCodec.transfer and pcc_attr_transfer_frames on the device: every result is held to the restatement
(tests/transfer_ref.py) bit for bit.  Each test first asserts, on the reference alone, that its input holds the case
it is there for.  tests/test_geometry_transfer.py has the rule worked by hand.
"""
import numpy as np
import pytest

import nn_ref
import transfer_ref
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def _check(geo, src, values, targets):
    """one frame through transfer with counts, against the restatement; -> (values, counts) of the reference"""
    want, want_cnt = transfer_ref.transfer_rows(src, values, targets)
    got, cnt = geo.transfer([src], [values], [targets], return_counts=True)
    assert len(got) == 1 and len(cnt) == 1
    _same(got[0], want)
    _same(cnt[0], want_cnt)
    return want, want_cnt


def _centres(points, k):
    cells = np.unique(points >> k, axis=0)
    return nn_ref.morton_sorted_unique((cells << k) + ((1 << k) >> 1)).astype(np.int32)


@pytest.fixture(scope="module")
def room():
    """room(4000, seed=3): its points (int32 [4000, 3]) and colours as uint8 RGB"""
    fr = pkg("workloads").room(4000, seed=3)
    return fr["points"].astype(np.int32), np.rint(fr["colors"] * 255.0).astype(np.uint8)


def _ties(queries, reference):
    """(how many queries reach their nearest distance at two rows of the reference or more, every query's first such
    row); the room's coordinates are below 2^9, so a squared distance fits int32"""
    q, r = np.asarray(queries, np.int32), np.asarray(reference, np.int32)
    n, rows = 0, []
    for a in range(0, q.shape[0], 1024):
        d = ((q[a:a + 1024, None, :] - r[None, :, :]) ** 2).sum(-1)
        n += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
        rows.append(d.argmin(1))
    return n, np.concatenate(rows)


def _wave_holds_aba(src, b):
    """some group of 64 rows of the Morton-sorted sources meets a target row in two separate runs; b: the target row of
    every source row as given"""
    b = b[np.argsort(nn_ref.morton_keys(src), kind="stable")]
    for g in range(0, b.shape[0], 64):
        w = b[g:g + 64]
        heads = w[np.concatenate([[True], w[1:] != w[:-1]])]
        if np.unique(heads).shape[0] < heads.shape[0]:
            return True
    return False


def test_hand_worked_stream(geo):
    src, values, targets, out, cnt = transfer_ref.hand_worked()
    want, want_cnt = _check(geo, src.astype(np.int32), values, targets.astype(np.int32))
    assert want.tolist() == out.tolist() == [2, 100, 9, 9, 50] and want_cnt.tolist() == cnt.tolist() == [2, 1, 2, 0, 1]


@pytest.mark.parametrize("lod, fallbacks, shared", [(1, 37, 49), (2, 77, 141), (3, 125, 383)])
def test_room_onto_its_cell_centres(geo, room, lod, fallbacks, shared):
    src, rgb = room
    targets = _centres(src, lod)
    _, cnt = _check(geo, src, rgb, targets)
    assert int((cnt == 0).sum()) == fallbacks >= 1 and int((cnt > 1).sum()) == shared >= 1
    assert np.abs(src).max() < 512
    backward, b = _ties(src, targets)
    assert backward >= 1 and _ties(targets, nn_ref.morton_sorted_unique(src))[0] >= 1
    assert np.array_equal(np.bincount(b, minlength=cnt.shape[0]), cnt) and _wave_holds_aba(src, b)


def test_target_denser_than_the_source(geo, room):
    src, rgb = room
    targets = nn_ref.morton_sorted_unique(np.concatenate([src[::2], src + (1, 0, 0), src[:50] + (0, 40, 0)])).astype(np.int32)
    assert targets.shape[0] == 6049
    _, cnt = _check(geo, src, rgb, targets)
    assert int((cnt == 0).sum()) > targets.shape[0] // 4


@pytest.mark.parametrize("fill", ["65535", "random"])
def test_one_hot_target(geo, fill):
    """70 000 uint16 rows on distinct points, one target: every lane of every wave adds to one address; the count
    leaves 16 bits and the sum 32"""
    n = 70_000
    i = np.arange(n)
    src = np.stack([i % 50 - 25, (i // 50) % 50 - 25, i // 2500], 1).astype(np.int32)
    assert np.unique(src, axis=0).shape[0] == n
    values = np.full(n, 65535, np.uint16) if fill == "65535" else np.random.default_rng(5).integers(0, 65536, n).astype(np.uint16)
    total = int(values.astype(np.int64).sum())
    assert n > 1 << 16 and (fill != "65535" or total > 1 << 32)
    target = np.array([[3, -2, 9]], np.int32)
    got, cnt = geo.transfer([src], [values], [target], return_counts=True)
    _same(got[0], np.array([(total + n // 2) // n], np.uint16))
    _same(cnt[0], np.array([n], np.uint32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_waves_and_runs_across_a_wave_boundary(geo, n):
    rng = np.random.default_rng(100 + n)
    src = np.stack([np.arange(n), np.zeros(n, int), np.zeros(n, int)], 1).astype(np.int32)      # Morton order is x order
    values = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    targets = np.array([[0, 0, 0], [n // 2, 0, 1], [n, 1, 0]], np.int32)
    targets = nn_ref.morton_sorted_unique(targets).astype(np.int32)
    assert targets.shape[0] == 3
    _, cnt = _check(geo, src, values, targets)
    assert int(cnt.sum()) == n
    if n > 64:      # a run of equal target rows spans lanes 63 and 64 of the sorted sources
        _, b = nn_ref.nn(src, targets)
        assert b[63] == b[64]


def test_frames_do_not_mix(geo):
    """three frames in one call, frame 1 empty on both sides, frames 0 and 2 the same coordinates with other values"""
    rng = np.random.default_rng(23)
    src = rng.integers(-20, 20, (300, 3)).astype(np.int32)
    t0 = _centres(src, 1)
    t2 = _centres(src, 2)
    v0 = rng.integers(0, 256, (300, 3)).astype(np.uint8)
    v2 = (255 - v0).astype(np.uint8)
    none = np.zeros((0, 3), np.int32)
    frames, values, targets = [src, none, src], [v0, np.zeros((0, 3), np.uint8), v2], [t0, none, t2]
    assert t0.shape[0] != t2.shape[0] != 300
    want, want_cnt = transfer_ref.transfer_frames(frames, values, targets)
    assert not np.array_equal(want[0][:8], want[2][:8])
    got, cnt = geo.transfer(frames, values, targets, return_counts=True)
    for f in range(3):
        _same(got[f], want[f])
        _same(cnt[f], want_cnt[f])
    assert got[1].shape == (0, 3) and cnt[1].shape == (0,)
    # a frame with sources and no targets, and a call whose frames are all without targets
    got = geo.transfer([src, src], [v0, v2], [none, t2])
    assert got[0].shape == (0, 3) and got[0].dtype == np.uint8
    _same(got[1], want[2])
    got, cnt = geo.transfer([src, none], [v0[:, 0], np.zeros((0, 2), np.uint16)], [none, none], return_counts=True)
    assert [g.shape for g in got] == [(0,), (0, 2)] and [g.dtype for g in got] == [np.uint8, np.uint16]
    assert [c.shape for c in cnt] == [(0,), (0,)] and cnt[0].dtype == np.uint32
    # uint8 RGB beside a 1-D uint16 frame in one call, on the host and on the device
    import torch
    v16 = rng.integers(0, 65536, 300).astype(np.uint16)
    mixed = transfer_ref.transfer_frames([src, src], [v0, v16], [t0, t2])[0]
    got = geo.transfer([src, src], [v0, v16], [t0, t2])
    dev = lambda a: torch.from_numpy(a).to(geo.rt.device)      # noqa: E731
    on_dev = geo.transfer([dev(src), dev(src)], [v0, v16], [dev(t0), dev(t2)], output="device")
    for f in range(2):
        _same(got[f], mixed[f])
        _same(on_dev[f].cpu().numpy(), mixed[f])
    assert geo.transfer([], [], []) == [] and geo.transfer([], [], [], return_counts=True) == ([], [])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("channels", [0, 1, 2, 3, 4])
def test_dtypes_and_channels(geo, dtype, channels):
    """channels 0: a 1-D [n] input, which gives [n_to] back"""
    rng = np.random.default_rng(31 + channels)
    src = rng.integers(-12, 12, (500, 3)).astype(np.int32)
    shape = (500,) if channels == 0 else (500, channels)
    values = rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    targets = _centres(src, 1)
    want, cnt = _check(geo, src, values, targets)
    assert want.shape == ((targets.shape[0],) if channels == 0 else (targets.shape[0], channels))
    assert (cnt == 0).any() and (cnt > 1).any()


def test_rows_as_given_and_device_frames(geo):
    import torch
    rng = np.random.default_rng(43)
    base = rng.integers(-10, 10, (400, 3)).astype(np.int32)
    # duplicate rows; (50, 50, 50) twice between two targets: one takes both rows, the other falls back on the point
    src = np.concatenate([base, base[rng.integers(0, 400, 150)], [[50, 50, 50]] * 2]).astype(np.int32)
    src = src[rng.permutation(src.shape[0])]
    values = rng.integers(0, 65536, (src.shape[0], 2)).astype(np.uint16)
    cells = np.concatenate([_centres(base, 1), [[50, 50, 49], [50, 50, 51]]])
    rows = cells[rng.integers(0, cells.shape[0], cells.shape[0] + 70)]      # shuffled, with duplicate rows
    rows = np.concatenate([rows, cells]).astype(np.int32)
    want, want_cnt = transfer_ref.transfer_rows(src, values, rows)
    # a duplicated source point is some target's fallback
    distinct, _ = transfer_ref.merged(src, values)
    t = nn_ref.morton_sorted_unique(rows)
    _, f = nn_ref.nn(t, distinct)
    _, cnt_t = transfer_ref.transfer(src, values, t)
    dup = np.array([(src == p).all(1).sum() for p in distinct]) > 1
    assert (dup[f] & (cnt_t == 0)).any()
    assert np.unique(rows, axis=0).shape[0] < rows.shape[0]
    got, cnt = geo.transfer([src], [values], [rows], return_counts=True)
    _same(got[0], want)
    _same(cnt[0], want_cnt)
    dev = geo.rt.device
    got, cnt = geo.transfer([torch.from_numpy(src).to(dev)], [values], [torch.from_numpy(rows).to(dev)], output="device",
                            return_counts=True)
    assert got[0].device == dev and got[0].dtype == torch.uint16 and cnt[0].dtype == torch.uint32
    _same(got[0].cpu().numpy(), want)
    _same(cnt[0].cpu().numpy(), want_cnt)
    with pytest.raises(ValueError, match="one side on the host"):
        geo.transfer([src], [values], [torch.from_numpy(rows).to(dev)])
    with pytest.raises(ValueError, match="output"):
        geo.transfer([src], [values], [rows], output="cuda")


def test_identities(geo, room):
    src, rgb = room
    rng = np.random.default_rng(47)
    pts = np.concatenate([src[:1500], src[rng.integers(0, 1500, 300)]])      # duplicates: the merge has work
    vals = rng.integers(0, 256, (pts.shape[0], 3)).astype(np.uint8)
    blobs, attr_blobs = geo.compress([pts], attributes=[vals])
    decoded, merged = geo.decompress(blobs, attr_blobs)
    got = geo.transfer([pts], [vals], [decoded[0]])
    _same(got[0], merged[0])
    # onto its own rows: every row its point's merged value
    own = geo.transfer([pts], [vals], [pts])[0]
    _same(own, transfer_ref.transfer_rows(pts, vals, pts)[0])
    # the same call twice: the same bytes
    targets = _centres(src, 2)
    a = geo.transfer([src], [rgb], [targets])[0]
    b = geo.transfer([src], [rgb], [targets])[0]
    assert a.tobytes() == b.tobytes()
    # and the chain closes: the result is an attribute side of distortion
    rep = geo.distortion([targets], [src], [a], [rgb])
    assert len(rep[0]["attr_mse_ab"]) == 3 and all(np.isfinite(rep[0]["attr_mse_ab"]))


def test_refusals_each_followed_by_a_clean_call(geo):
    src, values, targets, out, _ = transfer_ref.hand_worked()
    src, targets = src.astype(np.int32), targets.astype(np.int32)

    def clean():
        assert geo.transfer([src], [values], [targets])[0].tolist() == out.tolist()

    with pytest.raises(TypeError, match="float32 frames"):
        geo.transfer([src.astype(np.float32)], [values], [targets])
    clean()
    with pytest.raises(TypeError, match="float32 frames"):
        geo.transfer([src], [values], [targets.astype(np.float32)])
    clean()
    with pytest.raises(ValueError, match="1 frames against 2"):
        geo.transfer([src], [values], [targets, targets])
    clean()
    with pytest.raises(ValueError, match="frame 0: 5 attribute rows for 6 points"):
        geo.transfer([src], [values[:5]], [targets])
    clean()
    with pytest.raises(ValueError, match="1 attribute arrays for 2 frames"):
        geo.transfer([src, src], [values], [targets, targets])
    clean()
    none = np.zeros((0, 3), np.int32)
    with pytest.raises(ValueError, match="frame 1: 5 points against an empty source"):
        geo.transfer([src, none], [values, np.zeros(0, np.uint8)], [targets, targets])
    clean()


def test_c_abi_rows_out_of_range_and_empty_sides(rt):
    """row arrays holding -1 and rows at or behind their range add nothing and write nothing out of bounds (outputs
    with a canary tail); n_s == 0 zeroes the outputs, n_t == 0 touches nothing"""
    import ctypes as C

    import torch
    rtm = pkg("runtime")
    rng = np.random.default_rng(61)
    n_s, n_t, c = 200, 40, 3
    src = np.stack([np.arange(n_s) // 2, np.zeros(n_s, int), np.zeros(n_s, int)], 1)      # every point twice, sorted
    skeys = nn_ref.morton_keys(src)
    sruns = np.arange(0, n_s, 2).astype(np.uint32)
    n_su = sruns.shape[0]
    values = rng.integers(0, 65536, (n_s, c)).astype(np.uint16)
    row_st = rng.integers(0, n_t, n_s).astype(np.int32)
    row_st[::7] = -1
    row_st[3::11] = n_t
    row_st[5::13] = 1 << 30
    row_st[row_st == 17] = 18      # target 17 is nobody's: a fallback
    row_ts = rng.integers(0, n_su, n_t).astype(np.int32)
    row_ts[4], row_ts[9], row_ts[20] = -1, n_su, 1 << 30
    row_st[row_st == 4] = -1      # so that the fallbacks with rows out of range are taken
    row_st[row_st == 9] = n_t + 5
    row_st[row_st == 20] = -7
    ok = (row_st >= 0) & (row_st < n_t)
    sums = np.zeros((n_t, c), np.int64)
    np.add.at(sums, row_st[ok], values[ok].astype(np.int64))
    cnt = np.bincount(row_st[ok], minlength=n_t).astype(np.int64)[:, None]
    want = (sums + cnt // 2) // np.maximum(cnt, 1)
    for t in np.flatnonzero(cnt[:, 0] == 0):
        u = row_ts[t]
        pair = values[2 * u:2 * u + 2].astype(np.int64) if 0 <= u < n_su else np.zeros((2, c), np.int64)
        want[t] = (pair.sum(0) + 1) // 2
    assert cnt[17, 0] == 0 and want[17].any() and not want[[4, 9, 20]].any() and (cnt[:, 0] > 1).any()

    dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).to(rt.device)      # noqa: E731
    tail, canary = 4096, 0xA5A5
    fresh = lambda: torch.from_numpy(np.full(n_t * c + tail, canary, np.uint16)).to(rt.device)      # noqa: E731
    out = fresh()
    d_skeys, d_sruns, d_values, d_st, d_ts = dev(skeys), dev(sruns), dev(values), dev(row_st), dev(row_ts)
    _, count = rt.attr_transfer_frames(d_skeys, d_sruns, n_su, d_values, d_st, d_ts, 1, out=out)
    rt.sync()
    o = out.cpu().numpy()
    assert np.array_equal(o[:n_t * c].reshape(n_t, c), want.astype(np.uint16)) and np.all(o[n_t * c:] == canary)
    assert np.array_equal(count.cpu().numpy().view(np.uint32), cnt[:, 0].astype(np.uint32))
    # a source key of a frame outside the call adds nothing, in either kernel
    far = skeys.copy()
    far[:] |= np.uint64(1) << np.uint64(48)
    got, count = rt.attr_transfer_frames(dev(far), d_sruns, n_su, d_values, d_st, d_ts, 1)
    rt.sync()
    assert not got.cpu().numpy().any() and not count.cpu().numpy().any()
    # n_s == 0: zeros; n_t == 0: nothing is touched
    out = fresh()
    count = torch.full((n_t + tail,), 77, dtype=torch.int32, device=rt.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    rtm.check(rt.lib.pcc_attr_transfer_frames(rt.ctx, None, 0, None, 0, None, None, ptr(d_ts), n_t, 2, c, 1, ptr(out), ptr(count)),
              "pcc_attr_transfer_frames")
    rt.sync()
    o, k = out.cpu().numpy(), count.cpu().numpy()
    assert not o[:n_t * c].any() and np.all(o[n_t * c:] == canary) and not k[:n_t].any() and np.all(k[n_t:] == 77)
    out = fresh()
    rtm.check(rt.lib.pcc_attr_transfer_frames(rt.ctx, ptr(d_skeys), n_s, ptr(d_sruns), n_su, ptr(d_values), ptr(d_st), None, 0, 2, c, 1,
                                              ptr(out), None), "pcc_attr_transfer_frames")
    rt.sync()
    assert np.all(out.cpu().numpy() == canary)
    # the argument checks, in words
    for args, word in (((ptr(d_skeys), (1 << 27) + 1, ptr(d_sruns), n_su, ptr(d_values), ptr(d_st), ptr(d_ts), n_t, 2, c, 1), "bad argument"),
                       ((ptr(d_skeys), n_s, ptr(d_sruns), n_su, ptr(d_values), ptr(d_st), ptr(d_ts), n_t, 3, c, 1), "bpv=3"),
                       ((ptr(d_skeys), n_s, ptr(d_sruns), n_su, ptr(d_values), ptr(d_st), ptr(d_ts), n_t, 2, 5, 1), "channels=5"),
                       ((ptr(d_skeys), n_s, ptr(d_sruns), n_su, None, ptr(d_st), ptr(d_ts), n_t, 2, c, 1), "null source arrays"),
                       ((ptr(d_skeys), n_s, ptr(d_sruns), n_su, ptr(d_values), ptr(d_st), None, n_t, 2, c, 1), "null target arrays")):
        assert rt.lib.pcc_attr_transfer_frames(rt.ctx, *args, ptr(out), None) != 0
        assert word in rt.lib.pcc_last_error().decode()
