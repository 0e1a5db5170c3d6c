"""compress(..., predict="previous", history=K) on the GPU: the unions of the windows are formed by the merge kernels of
csrc/octree4.hip (pcc_merge_keys), on the encoder's side for every predicted frame of a call side by side, on the
decoder's frame after frame from the keys of the last decoded frames.  Every blob byte for byte against the helper of
octree_history_ref.py (the reference coder against the union, the window's frames - 1 in byte 3), every decode against
np.unique of the frame; then the merge alone against np.unique of the concatenated lists."""
import numpy as np
import pytest

import octree_history_ref as hist
import octree_inter_ref as ref4
from conftest import pkg, random_cloud
from test_geometry_calls import recorded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo(rt):
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _unique(p):
    return np.unique(np.asarray(p, np.int32), axis=0)


def _morton_sorted(p):
    p = _unique(p).reshape(-1, 3)
    return p[np.argsort(ref4.morton(p.astype(np.int64) + 32768), kind="stable")]


def _same(got, frames):
    return len(got) == len(frames) and all(np.array_equal(a, _morton_sorted(f)) for a, f in zip(got, frames))


# ------------------------------------------------------------------ chains of sweeps
@pytest.fixture(scope="module")
def sweeps(wl):
    return [f["points"].astype(np.int32) for f in wl.lidar_sequence(5, 16, 600)]


@pytest.fixture(scope="module")
def sweep_blobs():
    """the helper's blobs of the sweeps by (frame, W): computed once, shared by the cases"""
    return {}


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_chain_bytes_and_round_trip(geo, sweeps, sweep_blobs, K):
    G = type(geo)
    blobs = geo.compress(sweeps, predict="previous", history=K)
    plain = geo.compress(sweeps)
    want = hist.encode_chain(sweeps, K, v2=lambda p: None, cache=sweep_blobs)
    assert [G.reference_frames(b) for b in blobs] == [0] + [min(f, K) for f in range(1, 5)]
    assert blobs[0] == plain[0]
    for f in range(1, 5):
        assert blobs[f] == want[f], (K, f, len(blobs[f]), len(want[f]))
        merged = len(_unique(np.concatenate(sweeps[f - min(f, K):f])))
        assert G.geometry_info(blobs[f])["reference_points"] == merged
    if K == 1:
        assert blobs == geo.compress(sweeps, predict="previous")
    else:
        assert len(blobs[4]) < len(hist.encode_chain(sweeps, 1, cache=sweep_blobs)[4])      # what the window is for
    print("K = %d: bytes of the predicted sweeps" % K, [len(b) for b in blobs[1:]])
    assert _same(geo.decompress(blobs), sweeps)


def test_history_1_makes_the_call_of_before(geo, sweeps):
    frames = [f[:500] for f in sweeps[:3]]
    _, before = recorded(geo, lambda: geo.compress(frames, predict="previous"))
    for kw in ({"history": 1}, {"history": None}, {"history": 1, "reference": [frames[0]]}):
        _, calls = recorded(geo, lambda: geo.compress(frames, predict="previous", **kw))
        names = [c[0] for c in calls]
        assert "pcc_octree_encode_frames_inter" in names and "pcc_octree_encode_frames_inter_hist" not in names
        if "reference" not in kw:
            assert calls == before
    _, calls = recorded(geo, lambda: geo.compress(frames, predict="previous", history=2))
    assert "pcc_octree_encode_frames_inter_hist" in [c[0] for c in calls]


# ------------------------------------------------------------------ windows
@pytest.fixture(scope="module")
def chain():
    rng = np.random.default_rng(21)
    base = random_cloud(rng, 1500, extent=90, lo=-45)[:, 1:].astype(np.int32)
    return [np.concatenate([base[40 * f:1200 + 40 * f], base[:30]]) + np.array([f, 0, 0], np.int32) for f in range(6)]


def test_windows_under_an_intra_period(geo, chain):
    G = type(geo)
    blobs = geo.compress(chain, predict="previous", intra_period=3, history=3)
    assert [G.reference_frames(b) for b in blobs] == [0, 1, 2, 0, 1, 2]
    plain = geo.compress(chain)
    want = hist.encode_chain(chain, 3, intra_period=3, v2=lambda p: None)
    assert all(blobs[f] == (plain[f] if want[f] is None else want[f]) for f in range(6))
    assert _same(geo.decompress(blobs), chain)
    assert _same(geo.decompress(blobs[3:]), chain[3:])      # blob 3 is a random-access point: no window reaches past it


def test_windows_around_an_empty_frame(geo, chain):
    G = type(geo)
    frames = [chain[0], chain[1], chain[2], np.zeros((0, 3), np.int32), chain[3], chain[4], chain[5]]
    blobs = geo.compress(frames, predict="previous", history=3)
    assert [G.geometry_info(b)["version"] for b in blobs] == [2, 4, 4, 2, 2, 4, 4] and len(blobs[3]) == 24
    assert [G.reference_frames(b) for b in blobs] == [0, 1, 2, 0, 0, 1, 2]
    want = hist.encode_chain(frames, 3, v2=lambda p: None)
    assert all(want[f] is None or blobs[f] == want[f] for f in range(7))
    assert blobs[4] == geo.compress([chain[3]])[0]
    assert _same(geo.decompress(blobs), frames)


# ------------------------------------------------------------------ streaming: one frame per call
def test_streaming_against_the_last_two_frames(geo, chain):
    abi = pkg("_abi")
    f0, f1, f2 = chain[:3]
    blobs = geo.compress([f0, f1, f2], predict="previous", history=2)
    (one,) = geo.compress([f2], predict="previous", history=2, reference=[f0, f1])
    assert one == blobs[2] and one[3] == 1 and one == hist.encode_window(f2, [f0, f1])
    assert _same(geo.decompress([one], reference=[f0, f1]), [f2])
    assert _same(geo.decompress([one], reference=(chain[5], f0, f1)), [f2])      # more than the window: the last two count
    # a reference list of one frame at K = 2: a window of one
    (short,) = geo.compress([f2], predict="previous", history=2, reference=[f1])
    assert short == ref4.encode(f2, f1) and _same(geo.decompress([short], reference=[f1]), [f2])
    with pytest.raises(abi.PccError, match="frame 0.*needs 2 frames in front of it, 1 are here") as e:
        geo.decompress([one], reference=[f1])
    assert e.value.code == abi.PCC_E_ARG
    with pytest.raises(abi.PccError, match="frame 0") as e:      # one frame, given as before lists
        geo.decompress([one], reference=f1)
    assert e.value.code == abi.PCC_E_ARG
    with pytest.raises(abi.PccError, match="frame 0") as e:      # the window is there, the union is another
        geo.decompress([one], reference=[f1, f0 + 1])
    assert e.value.code == abi.PCC_E_ARG
    narrowed = bytearray(one)
    narrowed[3] = 0      # now it claims f1 alone: ref_n is the union's
    with pytest.raises(abi.PccError, match="frame 0") as e:
        geo.decompress([bytes(narrowed)], reference=[f0, f1])
    assert e.value.code == abi.PCC_E_ARG
    assert _same(geo.decompress([one], reference=[f0, f1]), [f2])      # the next call decodes
    widened = bytearray(one)
    widened[3] = 8       # a window of nine frames
    with pytest.raises(abi.PccError, match="frame 0") as e:
        geo.decompress([bytes(widened)], reference=[f0, f1])
    assert e.value.code == abi.PCC_E_STREAM
    assert type(geo).reference_frames(bytes(widened)) == 9      # the head is read as it is
    assert _same(geo.decompress(blobs), [f0, f1, f2])


def test_a_union_of_the_right_size_and_another_sum(geo, chain):
    """the host can only bound ref_n of a window; size and sum of the union are compared on the device"""
    abi = pkg("_abi")
    f0, f1, f2 = chain[:3]
    (one,) = geo.compress([f2], predict="previous", history=2, reference=[f0, f1])
    moved = f0.copy()
    moved[500, 2] += 1
    if len(_unique(np.concatenate([moved, f1]))) == len(_unique(np.concatenate([f0, f1]))):
        with pytest.raises(abi.PccError, match="frame 0.*differs") as e:
            geo.decompress([one], reference=[moved, f1])
        assert e.value.code == abi.PCC_E_ARG
    with pytest.raises(abi.PccError, match="frame 0.*differs") as e:      # inside the host's bounds, another size
        geo.decompress([one], reference=[np.delete(f0, slice(100, 105), 0), f1])
    assert e.value.code == abi.PCC_E_ARG
    assert _same(geo.decompress([one], reference=[f0, f1]), [f2])


# ------------------------------------------------------------------ what rides along
def test_lod_on_the_senders_side(geo, chain):
    frames = [f * 5 for f in chain[:3]]
    blobs = geo.compress(frames, lod=2, predict="previous", history=2)
    assert blobs[1] == ref4.encode(frames[1] >> 2, frames[0] >> 2, bias=32768 >> 2)
    assert blobs[2] == hist.encode_window(frames[2] >> 2, [frames[0] >> 2, frames[1] >> 2], bias=32768 >> 2)
    got = geo.decompress(blobs)
    assert np.array_equal(got[2], geo.decompress(geo.compress([frames[2]], lod=2))[0])


def test_device_frames_in_and_out(geo, chain):
    import torch
    dev = [torch.from_numpy(f).to(geo.rt.device) for f in chain[:4]]
    host = geo.compress(chain[:4], predict="previous", history=3)
    assert geo.compress(dev, predict="previous", history=3) == host
    assert geo.compress(dev[2:], predict="previous", history=3, reference=dev[:2]) == host[2:]
    got = geo.decompress(host, output="device")
    assert all(g.device == geo.rt.device for g in got) and _same([g.cpu().numpy() for g in got], chain[:4])
    got = geo.decompress(host[2:], output="device", reference=dev[:2])
    assert _same([g.cpu().numpy() for g in got], chain[2:4])


def test_float32_frames_and_return_index(geo, chain):
    voxel = 0.5
    fl = [(f.astype(np.float32) * np.float32(voxel)) for f in chain[:3]]
    want = geo.compress(chain[:3], predict="previous", history=2)
    assert geo.compress(fl, voxel=voxel, predict="previous", history=2) == want
    blobs, index = geo.compress(chain[:3], predict="previous", history=2, return_index=True)
    dec = geo.decompress(blobs)
    assert blobs == want and all(np.array_equal(dec[f][index[f]], chain[f]) for f in range(3))


def test_attributes_beside_a_history(geo, chain):
    rng = np.random.default_rng(4)
    frames = chain[:4]
    attrs = [rng.integers(0, 256, (f.shape[0], 3)).astype(np.uint8) for f in frames]
    blobs, ab = geo.compress(frames, attributes=attrs, predict="previous", history=3)
    plain, plain_ab = geo.compress(frames, attributes=attrs, predict="previous")
    assert ab == plain_ab and blobs[:2] == plain[:2] and blobs[2] != plain[2]
    pts, vals = geo.decompress(blobs, ab)
    ppts, pvals = geo.decompress(plain, plain_ab)
    assert all(np.array_equal(a, b) for a, b in zip(pts, ppts)) and all(np.array_equal(a, b) for a, b in zip(vals, pvals))


# ------------------------------------------------------------------ the merge alone
MASK48 = (1 << 48) - 1


def _merge(rt, lists, key_shift=0):
    """Runtime.merge_keys and what it must give: of the keys equal under (key & mask48) >> key_shift the one of the
    first list that holds it, in increasing order of that value"""
    import torch
    got = rt.merge_keys([torch.from_numpy(np.asarray(k, np.int64)).to(rt.device) for k in lists], key_shift).cpu().numpy()
    every = np.concatenate([np.asarray(k, np.int64) for k in lists])
    value = (every & MASK48) >> key_shift
    uniq, first = np.unique(value, return_index=True)      # the first occurrence: the earliest list
    assert got.dtype == np.int64 and got.shape == uniq.shape, (got.shape, uniq.shape)
    assert np.array_equal((got & MASK48) >> key_shift, uniq)
    assert np.array_equal(got, every[first])
    return got


def _sorted_keys(rng, n, hi=1 << 30):
    return np.sort(rng.choice(hi, n, replace=False)).astype(np.int64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_merge_list_lengths(rt, n):
    """either side of a wave and of a workgroup; the second list shares every third key of the first"""
    rng = np.random.default_rng(n)
    a = _sorted_keys(rng, n)
    b = np.unique(np.concatenate([a[::3], _sorted_keys(rng, n)]))
    _merge(rt, [a])
    _merge(rt, [a, b])
    _merge(rt, [b, a, a[: n // 2]])


def test_merge_special_lists(rt):
    rng = np.random.default_rng(7)
    a = _sorted_keys(rng, 700)
    assert np.array_equal(_merge(rt, [a, a.copy()]), a)                                   # two identical lists
    assert len(_merge(rt, [a[0::2], a[1::2]])) == 700                                     # disjoint, interleaved
    assert np.array_equal(_merge(rt, [a[350:], a[:350]]), a)                              # one wholly below another
    assert np.array_equal(_merge(rt, [a[:350], a[350:]]), a)
    _merge(rt, [a, a[:0], a[5:9]])                                                        # a list without keys


def test_merge_eight_lists_one_large(rt):
    """more than one tile of the scan (2048 elements), and lists of one key: in front of, inside, equal to and behind
    the large list's keys"""
    rng = np.random.default_rng(8)
    big = _sorted_keys(rng, 20000) + 10
    ones = [np.array([k], np.int64) for k in (0, int(big[0]), int(big[77]) + 1, int(big[9999]), int(big[-1]), int(big[-1]) + 5, 3)]
    _merge(rt, [big] + ones)
    _merge(rt, ones + [big])
    _merge(rt, ones[:3] + [big] + ones[3:])


def test_merge_keys_that_differ_only_above_bit_32(rt):
    low = np.array([5, 1 << 20, (1 << 32) - 1], np.int64)
    a = np.sort(np.concatenate([low, low + (1 << 32), low + (7 << 40)]))
    b = np.sort(np.concatenate([low + (1 << 33), low + (1 << 32), low + (1 << 47)]))
    got = _merge(rt, [a, b])
    assert len(got) == 15


def test_merge_carries_the_frame_bits_and_does_not_compare_them(rt):
    """an encode call's keys hold the frame index above bit 48: lists of frames 3, 1 and 2"""
    rng = np.random.default_rng(9)
    a = _sorted_keys(rng, 300, hi=1 << 24)
    b = np.unique(np.concatenate([a[::2], _sorted_keys(rng, 300, hi=1 << 24)]))
    c = np.unique(np.concatenate([b[::5], _sorted_keys(rng, 40, hi=1 << 24)]))
    got = _merge(rt, [a + (3 << 48), b + (1 << 48), c + (2 << 48)])
    assert np.array_equal(got & MASK48, np.unique(np.concatenate([a, b, c])))
    assert set((got >> 48).tolist()) == {1, 2, 3} and np.all((got >> 48)[np.isin(got & MASK48, a)] == 3)


def test_merge_under_a_key_shift(rt):
    """key_shift = 6: cells of 4 x 4 x 4 lattice points; every list holds one key per cell, as the front end leaves them"""
    rng = np.random.default_rng(10)

    def cells(n):
        k = _sorted_keys(rng, n, hi=1 << 22)
        return k[np.unique(k >> 6, return_index=True)[1]]
    lists = [cells(900), cells(900), cells(30)]
    got = _merge(rt, lists, key_shift=6)
    assert len(got) < sum(len(k) for k in lists) and len(got) == len(np.unique(np.concatenate(lists) >> 6))
