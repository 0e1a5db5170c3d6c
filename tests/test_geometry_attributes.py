"""Lossless per-point attributes beside the geometry blobs (attribute blob version 1, csrc/attr.hip;
pcc_attr_encode_frames / pcc_attr_decode_frames, Runtime.attr_*_frames, GeometryCodec(attributes=...)).  Every
attribute blob must equal the numpy restatement's (tests/attr_ref.py) bytes, and every decoded value the input after
the duplicate rule."""
import lzma
import os
import struct
import threading
import zlib

import numpy as np
import pytest

import attr_ref
from conftest import ROOT, pkg, random_cloud


def test_attr_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    for name in ("pcc_attr_encode_frames", "pcc_attr_decode_frames"):
        assert name + "(" in text
        assert name in abi.PROTOTYPES


def test_restatement_hand_worked_stream():
    """One point, one uint8 channel, value 5: pred 0, r = 5 = 0b101, k = 2.  Decisions (context: position in run's
    channel 0, bucket 0): zero flag 1 (0), sign 0 (1), prefix 1, 1, 0 (2, 3, 4), suffix bit 1 = 0 (2 + 7 + 1 = 10),
    bit 0 = 1 (9).  p0 = 4096 (2 c1 + 1) // (2 (c0 + c1 + 1)): a context that saw one one -> 3072, one zero -> 1024,
    nothing -> 2048.  rANS from x = 65536, decisions in reverse (freq 3072 each; start 1024 for a one):
      ctx 9 bit 1:  21 * 4096 + 1024 + 1024 = 88064      ctx 10 bit 0: 28 * 4096 + 2048 = 116736
      ctx 4 bit 0:  38 * 4096 + 0 = 155648               ctx 3 bit 1:  50 * 4096 + 2048 + 1024 = 207872
      ctx 2 bit 1:  67 * 4096 + 2048 + 1024 = 277504     ctx 1 bit 0:  90 * 4096 + 1024 = 369664
      ctx 0 bit 1: 120 * 4096 + 1024 + 1024 = 493568 = 0x00078800; no word (x < 3072 << 20)
    S = 1, one chunk of 192 words: lane 0's state, 63 states 0x00010000, 64 zero lengths."""
    p0 = [2048] * 80
    for k in (0, 2, 3, 9):
        p0[k] = 3072
    for k in (1, 4, 10):
        p0[k] = 1024
    body = struct.pack("<II", 1, 1) + struct.pack("<80H", *p0) + struct.pack("<I", 192)
    body += struct.pack("<128H", *([0x8800, 0x0007] + [0x0000, 0x0001] * 63)) + struct.pack("<64H", *([0] * 64))
    want = bytes([ord("A"), 1, 1, 1]) + struct.pack("<II", 1, len(body)) + body
    assert attr_ref.encode(np.array([5], np.uint8), 1) == want
    v, bpv = attr_ref.decode(want)
    assert bpv == 1 and v.tolist() == [[5]]
    assert attr_ref.encode(np.zeros((0, 3), np.uint8), 1) == bytes([ord("A"), 1, 1, 3]) + bytes(8)


@pytest.mark.parametrize("n,c,bpv", [(1, 1, 1), (2, 4, 2), (300, 1, 1), (64 * 512 + 1, 1, 1), (3000, 3, 1), (2000, 2, 2)])
def test_restatement_round_trip(n, c, bpv):
    rng = np.random.default_rng(n + 10 * c + bpv)
    hi = (1 << (8 * bpv)) - 1
    v = rng.integers(0, hi + 1, (n, c))
    v[::5] = 0
    v[1::5] = hi
    v[2::11] = v[1::11]
    v[3::13] = np.where(np.arange(v[3::13].size).reshape(v[3::13].shape) % 2, 0, hi)   # alternating extremes
    blob = attr_ref.encode(v, bpv)
    got, b = attr_ref.decode(blob)
    assert b == bpv and np.array_equal(got, v)


def test_restatement_rejects_a_damaged_stream():
    v = (np.arange(4000) * 7 % 251).astype(np.uint8)
    blob = bytearray(attr_ref.encode(v, 1))
    blob[-100] ^= 0x10
    with pytest.raises(AssertionError):
        got, _ = attr_ref.decode(bytes(blob))
        assert np.array_equal(got[:, 0], v)


# ------------------------------------------------------------------ GPU
def _pack(p):
    p = np.asarray(p, np.int64) + 32768
    return (p[:, 0] << 32) | (p[:, 1] << 16) | p[:, 2]


def _expected(pts, vals, decoded):
    u, mean = attr_ref.merge(np.asarray(pts, np.int32), vals)
    if decoded.shape[0] == 0:
        return mean[:0]
    idx = np.searchsorted(_pack(u), _pack(decoded))
    assert np.array_equal(u[idx], decoded)
    return mean[idx]


def _mixed(wl):
    rng = np.random.default_rng(41)
    sweep = wl.lidar_sweep(seed=1)["points"]
    room = wl.room(1_000_000, seed=0)
    dup = random_cloud(rng, 3000, extent=200, lo=-100)[:, 1:]
    dup = np.concatenate([dup, dup[:700], dup[::5]], 0)[rng.permutation(3000 + 700 + 600)]
    c64 = random_cloud(rng, 64 * 512 + 1, extent=400, lo=-200)[:, 1:]
    return [
        (sweep, wl.lidar_intensity(sweep, seed=1)),
        (room["points"], np.rint(255 * room["colors"]).astype(np.uint8)),
        (random_cloud(rng, 5000, extent=100, lo=-50)[:, 1:], rng.integers(0, 65536, 5000).astype(np.uint16)),
        (random_cloud(rng, 3000, extent=100, lo=-50)[:, 1:].astype(np.int16), rng.integers(0, 256, (3000, 4)).astype(np.uint8)),
        (np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8)),
        (random_cloud(rng, 1, extent=10)[:, 1:], np.array([[7, 65535]], np.uint16)),
        (random_cloud(rng, 2, extent=10)[:, 1:], np.array([255, 0], np.uint8)),
        (dup, rng.integers(0, 256, (dup.shape[0], 2)).astype(np.uint8)),
        (c64[:64 * 512], rng.integers(0, 256, 64 * 512).astype(np.uint8)),
        (c64, (np.arange(c64.shape[0]) % 256).astype(np.uint8)),
    ]


@pytest.fixture(scope="module")
def mixed(wl):
    geo = pkg().GeometryCodec()
    cases = _mixed(wl)
    frames = [p for p, _ in cases]
    attrs = [a for _, a in cases]
    blobs, ablobs = geo.compress(frames, attributes=attrs)
    yield geo, cases, blobs, ablobs
    geo.close()


@pytest.mark.gpu
def test_mixed_batch(mixed):
    geo, cases, blobs, ablobs = mixed
    frames = [p for p, _ in cases]
    assert blobs == geo.compress(frames)                                    # the geometry blobs as without attributes
    pts, got = geo.decompress(blobs, ablobs)
    dpts, dgot = geo.decompress(blobs, ablobs, output="device")
    for f, ((p, a), b, g) in enumerate(zip(cases, ablobs, got)):
        a2 = a if a.ndim == 2 else a[:, None]
        want = _expected(p, a2, pts[f])
        assert g.dtype == a.dtype and g.shape == (pts[f].shape[0], a2.shape[1]), f
        assert np.array_equal(g, want), f"frame {f}: decoded values differ"
        assert b == attr_ref.encode(want, a.dtype.itemsize), f"frame {f}: blob differs from the restatement's"
        assert dgot[f].is_cuda and np.array_equal(dgot[f].cpu().numpy(), want), f"frame {f}: device values differ"
    assert len(ablobs[4]) == 12


@pytest.mark.gpu
def test_rate(mixed):
    geo, cases, blobs, ablobs = mixed
    pts, got = geo.decompress(blobs, ablobs)
    for f in (0, 1):                                                       # sweep intensity, room RGB
        v = got[f]
        raw = v.tobytes()
        size = len(ablobs[f])
        assert size < len(zlib.compress(raw, 9)) and size < len(lzma.compress(raw, preset=9)), (f, size)
        assert size <= 1.10 * attr_ref.single_stream_bytes(v, 1) + 256, (f, size)


@pytest.mark.gpu
def test_corrupt_blobs_are_named_and_the_codec_stays_usable(mixed):
    abi = pkg("_abi")
    geo, cases, blobs, ablobs = mixed
    k = 3                                                                   # the c = 4 frame
    sub_g, sub_a = blobs[2:8], ablobs[2:8]
    want = geo.decompress(sub_g, sub_a)[1]
    kk = k - 2
    b = ablobs[k]

    def swapped(nb):
        return sub_a[:kk] + [nb] + sub_a[kk + 1:]
    cases_ = {f"header byte {i}": bytes(b[:i]) + bytes([b[i] ^ (1 << (i % 8))]) + bytes(b[i + 1:]) for i in range(20)}
    for i in (300, 700, len(b) // 2, len(b) - 3):
        cases_[f"payload byte {i}"] = bytes(b[:i]) + bytes([b[i] ^ 0x21]) + bytes(b[i + 1:])
    cases_["cut"] = bytes(b[:-2])
    cases_["cut header"] = bytes(b[:15])
    for what, nb in cases_.items():
        with pytest.raises(abi.PccError) as e:
            geo.decompress(sub_g, swapped(nb))
        assert f"frame {kk}:" in str(e.value), (what, str(e.value))
        got = geo.decompress(sub_g, sub_a)[1]
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), what
    # an attribute blob beside the geometry of a frame with another point count
    with pytest.raises(abi.PccError) as e:
        geo.decompress(sub_g, sub_a[:1] + [sub_a[2], sub_a[1]] + sub_a[3:])
    assert e.value.code == abi.PCC_E_STREAM and "frame 1:" in str(e.value)
    with pytest.raises(ValueError):
        geo.compress([cases[2][0]], attributes=[cases[2][1][:-1]])
    with pytest.raises(TypeError):
        geo.compress([cases[2][0]], attributes=[cases[2][1].astype(np.int32)])
    with pytest.raises(ValueError):
        geo.compress([cases[2][0]], attributes=[np.zeros((5000, 5), np.uint8)])


@pytest.mark.gpu
def test_two_codecs_on_two_threads(wl):
    GeometryCodec = pkg().GeometryCodec
    rng = np.random.default_rng(4)
    seqs = []
    for s in range(2):
        fr = [wl.lidar_sweep(32, 900, seed=s + 3)["points"] for _ in range(2)] + [random_cloud(rng, 4000, extent=80)[:, 1:]]
        seqs.append((fr, [wl.lidar_intensity(fr[0]), wl.lidar_intensity(fr[1], seed=2),
                          rng.integers(0, 256, (4000, 3)).astype(np.uint8)]))
    one = GeometryCodec()
    serial = [one.compress(f, attributes=a) for f, a in seqs]
    codecs = [GeometryCodec(), GeometryCodec()]
    got, errors = [None, None], []

    def run(i):
        try:
            for _ in range(3):
                out = codecs[i].compress(*seqs[i][:1], attributes=seqs[i][1])
            got[i] = out
        except Exception as exc:           # surfaced below
            errors.append(exc)
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == serial
    for c in codecs + [one]:
        c.close()
