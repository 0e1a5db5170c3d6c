"""Geometry-only coding of point-set sequences: B frames into B version-2 blobs in one call
(pcc_octree_encode_frames / pcc_octree_decode_frames, Runtime.octree_*_frames, GeometryCodec).  Every blob must be
byte-identical to the oracle's blob of that frame alone, and every decoded frame the oracle's points."""
import ctypes as C
import os
import struct
import threading

import numpy as np
import pytest

from conftest import ROOT, pkg, random_cloud


def _declared(name):
    return name in open(os.path.join(ROOT, "include", "pcc.h")).read()


def test_frames_abi_is_declared_and_bound():
    abi = pkg("_abi")
    for name in ("pcc_octree_encode_frames", "pcc_octree_decode_frames"):
        assert _declared(name + "(")
        assert name in abi.PROTOTYPES


def _cloud(rng, n, extent=200, lo=-100):
    return random_cloud(rng, n, extent=extent, lo=lo)[:, 1:].copy()


def _mixed_frames(wl):
    rng = np.random.default_rng(31)
    dup = _cloud(rng, 3000)
    dup = np.concatenate([dup, dup[:700], dup[::5]], 0)[rng.permutation(3000 + 700 + 600)]
    edge = np.array([[32767, 32767, 32767], [-32768, 5, 9], [-32767, -32767, -32767], [0, 0, 0], [32767, -32768, 1],
                     [-32767, 32767, -32767]], np.int32)
    neg = _cloud(rng, 5000, extent=300, lo=-30000)
    return [
        wl.lidar_sweep(seed=1)["points"],
        wl.lidar_sweep(32, 900, seed=2)["points"],
        np.zeros((0, 3), np.int16),
        wl.room(1_000_000, seed=0)["points"],
        _cloud(rng, 1), _cloud(rng, 2), _cloud(rng, 9),
        _cloud(rng, 65536, extent=400, lo=-200), _cloud(rng, 65537, extent=400, lo=-200),
        dup, neg.astype(np.int16), edge,
        np.zeros((0, 3), np.int32),
    ]


def _unique(pts):
    return np.unique(np.asarray(pts, np.int32).reshape(-1, 3), axis=0)


@pytest.mark.gpu
def test_mixed_batch_against_the_oracle(oracle, wl):
    geo = pkg().GeometryCodec()
    frames = _mixed_frames(wl)
    blobs = geo.compress(frames)
    assert len(blobs) == len(frames)
    refs = [oracle.octree_encode(_unique(f), 32768, version=2) for f in frames]
    for f, (b, r) in enumerate(zip(blobs, refs)):
        assert b == r, f"frame {f}: blob differs from the oracle's ({len(b)} vs {len(r)} bytes)"
    assert len(blobs[2]) == 24 and len(blobs[-1]) == 24
    want = [oracle.octree_decode(r) for r in refs]
    host = geo.decompress(blobs)
    dev = geo.decompress(blobs, output="device")
    for f, (w, h, d) in enumerate(zip(want, host, dev)):
        assert isinstance(h, np.ndarray) and h.dtype == np.int32 and h.shape == w.shape, f
        assert np.array_equal(h, w), f"frame {f}: host points differ"
        assert d.is_cuda and np.array_equal(d.cpu().numpy(), w), f"frame {f}: device points differ"
    geo.close()


def _keys(rt, pts, batch=None):
    import torch
    b = np.zeros((pts.shape[0], 1), np.int32) if batch is None else batch.reshape(-1, 1).astype(np.int32)
    coords = np.concatenate([b, pts.astype(np.int32)], 1)
    keys = rt.morton_keys(rt.to_device(coords))
    rt.sort_pairs(keys)
    torch.cuda.synchronize()
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 9])
def test_one_frame_equals_the_single_frame_path(rt, wl, shift):
    rng = np.random.default_rng(5 + shift)
    stride = 8 if shift else 1
    sets = [random_cloud(rng, n, extent=100, lo=-50, stride=stride)[:, 1:] for n in (20000, 70000)]
    if not shift:
        sets.append(wl.lidar_sweep(seed=3)["points"].astype(np.int32))
    for pts in sets:
        keys = _keys(rt, pts)
        one = rt.octree_encode_frames(keys, 1, shift)
        assert len(one) == 1 and one[0] == rt.octree_encode(keys, shift, version=2)


@pytest.mark.gpu
def test_batch_with_a_key_shift_against_the_oracle(rt, oracle):
    """keys of stride-8 coordinates coded with key_shift 9: frame f equals the oracle's blob of coordinates / 8 (bias
    32768 / 8), small and wave-form frames and an empty one in one call"""
    rng = np.random.default_rng(19)
    frames = [random_cloud(rng, n, extent=e, lo=-e // 2, stride=8)[:, 1:] if n else np.zeros((0, 3), np.int32)
              for n, e in ((3000, 60), (0, 1), (70000, 100), (1, 1), (20000, 400))]
    batch = np.concatenate([np.full(f.shape[0], i) for i, f in enumerate(frames)])
    keys = _keys(rt, np.concatenate(frames, 0), batch)
    blobs = rt.octree_encode_frames(keys, len(frames), 9)
    refs = [oracle.octree_encode(f // 8, 4096, version=2) for f in frames]
    assert blobs == refs
    for b, g in zip(blobs, rt.octree_decode_frames(blobs)):
        assert np.array_equal(g, oracle.octree_decode(b))


@pytest.mark.gpu
def test_coordinates_outside_int16_are_refused():
    abi = pkg("_abi")
    geo = pkg().GeometryCodec()
    bad = np.array([[0, 0, 0], [40000, 1, 2]], np.int32)
    with pytest.raises(abi.PccError) as e:
        geo.compress([np.zeros((5, 3), np.int32), bad])
    assert e.value.code == abi.PCC_E_RANGE
    pts = np.array([[1, 2, 3], [-4, 5, -6]], np.int16)
    assert geo.decompress(geo.compress([pts]))[0].shape == (2, 3)    # the codec stays usable
    geo.close()


@pytest.mark.gpu
def test_oracle_blobs_decode_in_one_call(rt, oracle):
    rng = np.random.default_rng(64)
    sizes = [int(v) for v in rng.integers(1, 4000, 60)] + [1, 2, 70000, 0]
    clouds = [_cloud(rng, n, extent=60 if n < 50000 else 300, lo=int(rng.integers(-20000, 20000))) if n else
              np.zeros((0, 3), np.int32) for n in sizes]
    blobs = [oracle.octree_encode(c, 32768, version=2) for c in clouds]
    got = rt.octree_decode_frames(blobs)
    assert len(got) == 64
    for f, (b, g) in enumerate(zip(blobs, got)):
        assert np.array_equal(g, oracle.octree_decode(b)), f
    dev = rt.octree_decode_frames(blobs, device=True)
    assert all(np.array_equal(d.cpu().numpy(), g) for d, g in zip(dev, got))


def _batch8(oracle):
    rng = np.random.default_rng(88)
    return [oracle.octree_encode(_cloud(rng, int(n), extent=120), 32768, version=2)
            for n in (3000, 800, 5000, 1, 2500, 4000, 600, 1800)]


@pytest.mark.gpu
def test_corrupt_frame_is_named_and_ctx_stays_usable(rt, oracle):
    abi = pkg("_abi")
    blobs = _batch8(oracle)
    want = [oracle.octree_decode(b) for b in blobs]
    k = 5
    depth = blobs[k][2]
    off_len = 24 + 4 * depth + 8 + 216 + 4          # one chunk: its table, then 128 state words, then len[64]

    def flipped(at, val):
        b = bytearray(blobs[k])
        b[at] = val(b[at])
        return blobs[:k] + [bytes(b)] + blobs[k + 1:]

    cases = {
        "header level_n": flipped(24 + 4, lambda v: v ^ 0x40),
        "header S": flipped(24 + 4 * depth + 1, lambda v: v ^ 0x08),
        "payload length table": flipped(off_len + 256 + 2 * 3, lambda v: (v + 1) & 0xFF),
        "payload truncated": blobs[:k] + [blobs[k][:-2]] + blobs[k + 1:],
    }
    for what, batch in cases.items():
        with pytest.raises(abi.PccError) as e:
            rt.octree_decode_frames(batch)
        assert e.value.code == abi.PCC_E_STREAM, what
        assert f"frame {k}:" in str(e.value), (what, str(e.value))
        got = rt.octree_decode_frames(blobs)      # the next call on the same ctx
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), what


@pytest.mark.gpu
def test_tiny_payload_with_huge_levels_is_refused(rt, oracle):
    abi = pkg("_abi")
    blob = bytearray(_batch8(oracle)[0])
    depth = blob[2]
    struct.pack_into("<I", blob, 4, 0x7FFFFFFF)                      # points
    for L in range(1, depth):                                         # every level 8x its parent
        struct.pack_into("<I", blob, 24 + 4 * L, min(8 ** L, 0x7FFFFFFF))
    with pytest.raises(abi.PccError) as e:
        rt.octree_decode_frames([bytes(blob)])
    assert e.value.code == abi.PCC_E_STREAM and "frame 0:" in str(e.value)
    # S beyond the encoder's 512 nodes per lane: refused by the header check alone
    blob = bytearray(_batch8(oracle)[2])
    struct.pack_into("<I", blob, 24 + 4 * blob[2], 1024)
    with pytest.raises(abi.PccError) as e:
        rt.octree_decode_frames([_batch8(oracle)[1], bytes(blob)])
    assert e.value.code == abi.PCC_E_STREAM and "frame 1:" in str(e.value)
    assert "chunks of 64 x 1024" in str(e.value)                     # the header check, not a later one


@pytest.mark.gpu
def test_other_blob_versions_are_refused(rt, oracle):
    abi = pkg("_abi")
    blobs = _batch8(oracle)
    rng = np.random.default_rng(3)
    v1 = oracle.octree_encode(_cloud(rng, 500), 32768, version=1)
    with pytest.raises(abi.PccError) as e:
        rt.octree_decode_frames(blobs[:3] + [v1] + blobs[3:])
    assert e.value.code == abi.PCC_E_ARG and "frame 3:" in str(e.value)
    assert len(rt.octree_decode_frames(blobs)) == 8


@pytest.mark.gpu
def test_encode_capacity_and_key_checks(rt, wl):
    import torch
    abi = pkg("_abi")
    rng = np.random.default_rng(9)
    frames = [_cloud(rng, 4000), _cloud(rng, 70000, extent=400)]
    batch = np.concatenate([np.full(f.shape[0], i) for i, f in enumerate(frames)])
    keys = _keys(rt, np.concatenate(frames, 0), batch)
    n = keys.shape[0]
    blobs = rt.octree_encode_frames(keys, 2)
    need = sum(len(b) for b in blobs)
    offs = (C.c_int64 * 3)()
    for cap in (0, need - 1, len(blobs[0])):
        out = np.full(need + 256, 0xAB, np.uint8)
        rc = rt.lib.pcc_octree_encode_frames(rt.ctx, keys.data_ptr(), n, 2, 0, out.ctypes.data, cap, offs)
        assert rc == abi.PCC_E_NOMEM, cap
        assert np.all(out == 0xAB), cap                               # nothing written, let alone past cap
    out = np.empty(need, np.uint8)
    assert rt.lib.pcc_octree_encode_frames(rt.ctx, keys.data_ptr(), n, 2, 0, out.ctypes.data, need, offs) == 0
    assert [out[offs[f]:offs[f + 1]].tobytes() for f in range(2)] == blobs
    # a duplicate key, keys out of order, a frame index beyond n_frames
    dup = keys.clone()
    dup[1000] = dup[999]
    with pytest.raises(abi.PccError) as e:
        rt.octree_encode_frames(dup, 2)
    assert e.value.code == abi.PCC_E_DUP
    unsorted = keys.clone()
    unsorted[[10, 11]] = unsorted[[11, 10]]
    with pytest.raises(abi.PccError) as e:
        rt.octree_encode_frames(unsorted, 2)
    assert e.value.code == abi.PCC_E_ARG
    with pytest.raises(abi.PccError) as e:
        rt.octree_encode_frames(keys, 1)
    assert e.value.code == abi.PCC_E_ARG
    torch.cuda.synchronize()
    assert rt.octree_encode_frames(keys, 2) == blobs                 # the ctx is still good


@pytest.mark.gpu
def test_two_codecs_on_two_threads(wl):
    GeometryCodec = pkg().GeometryCodec
    rng = np.random.default_rng(2)
    seqs = [[wl.lidar_sweep(32, 900, seed=s)["points"] for s in range(4)] + [_cloud(rng, 9000)],
            [_cloud(rng, int(n), extent=150) for n in (70000, 10, 3000)] + [wl.lidar_sweep(seed=7)["points"]]]
    one = GeometryCodec()
    serial = [one.compress(s) for s in seqs]
    serial_pts = [one.decompress(b) for b in serial]
    codecs = [GeometryCodec(), GeometryCodec()]
    got = [None, None]
    errors = []

    def run(i):
        try:
            for _ in range(3):
                b = codecs[i].compress(seqs[i])
                p = codecs[i].decompress(b)
            got[i] = (b, p)
        except Exception as exc:           # surfaced below
            errors.append(exc)
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert got[i][0] == serial[i]
        assert all(np.array_equal(a, b) for a, b in zip(got[i][1], serial_pts[i]))
    for c in codecs + [one]:
        c.close()
