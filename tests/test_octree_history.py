"""compress(..., predict="previous", history=K): a predicted frame coded against the union of the up to K frames in
front of it (include/pcc.h has the window rule; the blob is version 4 with the window's frames - 1 in byte 3).  CPU
part: the helper of octree_history_ref.py against the reference coder's own decoder, the window rule, the byte counts
the feature was proposed with, the argument checks of the new keyword and reference_frames."""
import numpy as np
import pytest

import octree_history_ref as hist
import octree_inter_ref as ref4
from conftest import pkg, random_cloud


def _geo_class():
    return pkg("geometry").GeometryCodec


def _clouds(n, seed=21, size=300):
    rng = np.random.default_rng(seed)
    base = random_cloud(rng, size, extent=40, lo=-20)[:, 1:]
    return [base + rng.integers(-1, 2, base.shape) for _ in range(n)]


# ------------------------------------------------------------------ the helper
@pytest.mark.parametrize("w", [1, 2, 3, 8])
def test_reference_decoder_inverts_the_helper(w):
    frames = _clouds(w + 1)
    blob = hist.encode_window(frames[-1], frames[:-1])
    assert blob[:2] == b"O\x04" and blob[3] == w - 1
    # byte 3 apart, the blob is the reference coder's against the union
    merged = np.unique(np.concatenate(frames[:-1]), axis=0)
    plain = ref4.encode(frames[-1], merged)
    assert blob[:3] == plain[:3] and plain[3] == 0 and blob[4:] == plain[4:]
    h = ref4.header(blob)
    assert h["ref_n"] == len(merged) and max(len(np.unique(f, axis=0)) for f in frames[:-1]) <= h["ref_n"]
    dec = hist.decode_window(blob, frames[:-1])
    assert np.array_equal(np.unique(dec, axis=0), np.unique(frames[-1], axis=0))
    # more frames at hand than the window: the last W count
    assert np.array_equal(hist.decode_window(blob, _clouds(2, seed=5) + frames[:-1]), dec)
    if w > 1:
        with pytest.raises(ValueError, match="frames in front"):
            hist.decode_window(blob, frames[1:-1])
        with pytest.raises(ValueError, match="differs"):      # another window: another union
            hist.decode_window(blob, _clouds(1, seed=5) + frames[1:-1])


def test_a_window_of_one_is_the_blob_of_before():
    f0, f1 = _clouds(2)
    assert hist.encode_window(f1, [f0]) == ref4.encode(f1, f0)


def test_the_union_does_not_depend_on_order_or_repeats():
    f = _clouds(4)
    a = hist.encode_window(f[3], f[:3])
    assert a == hist.encode_window(f[3], [f[2], f[0], np.concatenate([f[1], f[0][:7]])])


# ------------------------------------------------------------------ the window rule
def test_windows_grow_up_to_history():
    n = [10] * 6
    assert hist.windows(n, 1) == [0, 1, 1, 1, 1, 1]
    assert hist.windows(n, 3) == [0, 1, 2, 3, 3, 3]
    assert hist.windows(n, 8) == [0, 1, 2, 3, 4, 5]


def test_windows_stop_at_an_intra_frame_which_may_be_in_them():
    n = [10] * 8
    assert hist.windows(n, 3, intra_period=3) == [0, 1, 2, 0, 1, 2, 0, 1]
    assert hist.windows(n, 2, intra_period=4) == [0, 1, 2, 2, 0, 1, 2, 2]
    assert hist.windows(n, 8, intra_period=1) == [0] * 8


def test_windows_stop_at_a_frame_without_points():
    assert hist.windows([10, 10, 10, 0, 10, 10, 10, 10], 3) == [0, 1, 2, None, 0, 1, 2, 3]
    assert hist.windows([0, 10, 10], 3) == [None, 0, 1]


def test_windows_over_reference_frames():
    """only the trailing run of non-empty reference frames exists, at most K of them count"""
    assert hist.windows([10, 10, 10, 10], 2, n_ref_frames=2) == [2, 2]
    assert hist.windows([10, 10, 10, 10], 3, n_ref_frames=2) == [2, 3]
    assert hist.windows([10, 0, 10, 10, 10], 3, n_ref_frames=3) == [1, 2]
    assert hist.windows([10, 10, 0, 10, 10], 3, n_ref_frames=3) == [0, 1]      # behind an empty reference: intra
    assert hist.windows([10, 10, 10], 2, intra_period=2, n_ref_frames=1) == [0, 1]      # coded frame 0 is intra: the reference is unused


def test_chain_helper_follows_the_rule():
    frames = _clouds(5, size=60)
    frames[2] = frames[2][:0]
    blobs = hist.encode_chain(frames, 3)
    assert [None if b is None else b[3] + 1 for b in blobs] == [None, 1, None, None, 1]
    blobs = hist.encode_chain(frames[3:], 2, references=frames[:2])
    assert [b[3] + 1 for b in blobs] == [2, 2]
    assert blobs[0] == hist.encode_window(frames[3], frames[:2]) and blobs[1] == hist.encode_window(frames[4], [frames[1], frames[3]])


# ------------------------------------------------------------------ the byte counts of the proposal
BYTES = {(0, 0, 0): {1: 9312, 2: 8508, 3: 8104}, (10, 0, 0): {1: 10348, 2: 9696, 3: 9378}}


@pytest.mark.parametrize("velocity", list(BYTES))
def test_bytes_of_a_sweep_against_the_last_k_sweeps(wl, velocity):
    frames = [f["points"].astype(np.int32) for f in wl.lidar_sequence(4, 16, 600, velocity=velocity)]
    got = {k: len(hist.encode_window(frames[3], frames[3 - k:3])) for k in (1, 2, 3)}
    print("frame 3 of lidar_sequence(4, 16, 600, velocity=%r): bytes at K = 1, 2, 3:" % (velocity,), got)
    assert got == BYTES[velocity]


# ------------------------------------------------------------------ host-only interfaces
def test_reference_frames():
    G = _geo_class()
    f = _clouds(4, size=40)
    assert G.reference_frames(bytes([ord("O"), 2]) + bytes(22)) == 0
    assert G.reference_frames(ref4.encode(f[1], f[0])) == 1
    assert G.reference_frames(hist.encode_window(f[3], f[:3])) == 3
    assert G.reference_frames(bytearray(hist.encode_window(f[3], f[1:3]))[:4]) == 2      # the head alone
    for bad in (b"", b"O\x04\x05", b"O\x01\x05\x00" + bytes(20), b"X\x04\x05\x00"):
        with pytest.raises(ValueError):
            G.reference_frames(bad)


def test_geometry_info_says_the_size_of_the_union():
    f = _clouds(3, size=40)
    info = _geo_class().geometry_info(hist.encode_window(f[2], f[:2]))
    assert info == {"version": 4, "points": len(np.unique(f[2], axis=0)), "predicted": True,
                    "reference_points": len(np.unique(np.concatenate(f[:2]), axis=0))}


def test_argument_checks_of_history():
    """raised before anything touches the device"""
    G = _geo_class()
    geo = G.__new__(G)                # no Runtime: the checks come first
    f = [np.zeros((2, 3), np.int16)]
    r = np.ones((2, 3), np.int16)
    for bad in (True, False, 2.0, "3", [2]):
        with pytest.raises(TypeError, match="history"):
            geo.compress(f, predict="previous", history=bad)
    for bad in (0, -1, 9, 100):
        with pytest.raises(ValueError, match="history"):
            geo.compress(f, predict="previous", history=bad)
    with pytest.raises(ValueError, match="history"):
        geo.compress(f, history=2)
    with pytest.raises(ValueError, match="reference"):
        geo.compress(f, predict="previous", history=2, reference=[r, r, r])      # more than K
    with pytest.raises(ValueError, match="reference"):
        geo.compress(f, predict="previous", reference=[r, r])                     # K = 1
    with pytest.raises(ValueError, match="reference"):
        geo.compress(f, predict="previous", history=2, reference=[])
    with pytest.raises(ValueError, match="reference: frame 1"):
        geo.compress(f, predict="previous", history=2, reference=[r, np.zeros((2, 2), np.int16)])
    with pytest.raises(ValueError, match="reference"):
        geo.compress(f, predict="previous", history=2, reference=(r, r.astype(np.float32)))
    with pytest.raises(ValueError, match="reference"):
        geo.decompress([b""], reference=[r.astype(np.int32)] * 9)
    with pytest.raises(ValueError, match="reference"):
        geo.decompress([b""], reference=[])
    with pytest.raises((TypeError, ValueError), match="reference"):
        geo.decompress([b""], reference=[r.astype(np.float32)])
