"""Levels of detail of version-2 geometry blobs (csrc/octree2_blob.h, pcc_octree_lod_info /
pcc_octree_decode_frames_lod, GeometryCodec.lod_info / decompress(lod=) / compress(lod=)): a prefix of a stored blob
decodes to the distinct cells points >> k in Morton order, and compress(lod=k) writes the blob of those cells."""
import os
import struct
import threading

import numpy as np
import pytest

import attr_ref
import octree2_layout_ref
from conftest import ROOT, pkg
from test_geometry_frames import _cloud, _mixed_frames, _unique

LODS = (0, 1, 2, 3, 5, 9, 15)


# ------------------------------------------------------------------ the rule, restated from the blob's bytes alone
def _rule(blob, k):
    """(bytes, cells) of level of detail k, read off the bytes of a well-formed version-2 blob (the restatement of the
    rule is octree2_layout_ref.plan: one copy for this file and for the tests of the decoder under forced layouts)"""
    p = octree2_layout_ref.plan(blob, k)
    return p["bytes"], p["cells"]


def _cells(points, k):
    return np.unique(np.asarray(points, np.int32).reshape(-1, 3) >> k, axis=0)


def _grid_cloud(rng, n, extent, lo):
    idx = rng.choice(extent ** 3, n, replace=False)
    return (np.stack([idx // extent ** 2, idx // extent % extent, idx % extent], 1) + lo).astype(np.int32)


EDGE = np.array([[32767, 32767, 32767], [-32768, 5, 9], [-32767, -32767, -32767], [0, 0, 0], [32767, -32768, 1],
                 [-32767, 32767, -32767]], np.int32)


@pytest.fixture(scope="module")
def host_cases(oracle, wl):
    rng = np.random.default_rng(77)
    clouds = {
        "sweep": wl.lidar_sweep(seed=1)["points"],
        "sweep 32 x 900": wl.lidar_sweep(32, 900, seed=2)["points"],
        "room": wl.room(1_000_000, seed=0)["points"],
        "depth 6": _grid_cloud(rng, 70000, 64, 0),
        "depth 9": _grid_cloud(rng, 70000, 300, -30000),
        "one point": np.array([[-7, 300, 12]], np.int32),
        "empty": np.zeros((0, 3), np.int32),
        "int16 corners": EDGE,
    }
    return {name: (_unique(p), oracle.octree_encode(_unique(p), 32768, version=2)) for name, p in clouds.items()}


def test_lod_abi_is_declared_and_bound():
    abi = pkg("_abi")
    header = open(os.path.join(ROOT, "include", "pcc.h")).read()
    for name in ("pcc_octree_lod_info", "pcc_octree_decode_frames_lod"):
        assert name + "(" in header
        assert name in abi.PROTOTYPES
    assert hasattr(abi.lib(), "pcc_octree_lod_info")


def test_lod_info_against_the_rule(host_cases):
    GeometryCodec = pkg().GeometryCodec
    assert host_cases["depth 6"][1][2] == 6 and host_cases["depth 9"][1][2] == 9 and host_cases["int16 corners"][1][2] == 16
    for name, (pts, blob) in host_cases.items():
        prev = None
        for k in range(16):
            nbytes, cells = GeometryCodec.lod_info(blob, k)
            assert (nbytes, cells) == _rule(blob, k), (name, k)
            assert cells == _cells(pts, k).shape[0], (name, k)
            assert nbytes <= len(blob) and (k > 0 or nbytes == len(blob)), (name, k)
            assert prev is None or nbytes <= prev, (name, k)
            # the same answer from exactly the prefix of the next finer level
            finer = GeometryCodec.lod_info(blob, max(k - 1, 0))[0]
            assert GeometryCodec.lod_info(blob[:finer], k) == (nbytes, cells), (name, k)
            prev = nbytes


def test_lod_shares_of_the_sweep_and_the_room(host_cases):
    """the figures DESIGN.md 6c quotes: cells and the prefix's share of the blob"""
    GeometryCodec = pkg().GeometryCodec
    want = {"sweep": [(91627, 0.578), (53723, 0.262), (30955, 0.130), (14341, 0.061)],
            "room": [(407830, 0.177), (105749, 0.049), (26386, 0.018), (6555, 0.008)],
            "sweep 32 x 900": [(25655, 0.660), (17629, 0.356), (11182, 0.207), (6102, 0.115)]}
    for name, rows in want.items():
        blob = host_cases[name][1]
        for k, (cells, share) in enumerate(rows, 1):
            nbytes, m = GeometryCodec.lod_info(blob, k)
            assert m == cells and round(nbytes / len(blob), 3) == share, (name, k, m, nbytes / len(blob))


def test_lod_info_refusals(host_cases, oracle):
    abi = pkg("_abi")
    GeometryCodec, Runtime = pkg().GeometryCodec, pkg("runtime").Runtime
    blob = host_cases["sweep"][1]
    for bad in (16, -1, 1.5, True):
        with pytest.raises(ValueError):
            GeometryCodec.lod_info(blob, bad)
    for bad in (16, -1):
        with pytest.raises(abi.PccError) as e:
            Runtime.octree_lod_info(blob, bad)
        assert e.value.code == abi.PCC_E_ARG
    v1 = oracle.octree_encode(host_cases["depth 6"][0][:500], 32768, version=1)
    with pytest.raises(abi.PccError) as e:
        GeometryCodec.lod_info(v1, 1)
    assert e.value.code == abi.PCC_E_ARG
    d, nc = blob[2], struct.unpack_from("<I", blob, 24 + 4 * blob[2] + 4)[0]
    off_table = 24 + 4 * d + 8 + 216
    assert nc >= 2
    for cut in (off_table + 2, off_table + 4 * nc - 1, off_table - 10, 30, 23):
        with pytest.raises(abi.PccError) as e:
            GeometryCodec.lod_info(blob[:cut], 3)
        assert e.value.code == abi.PCC_E_STREAM, cut
    # short of the last needed chunk's length table, and just long enough for it
    need, _ = GeometryCodec.lod_info(blob, 4)
    table_end = off_table + 4 * nc + 2 * 192
    assert need > table_end
    with pytest.raises(abi.PccError) as e:
        GeometryCodec.lod_info(blob[:table_end - 1], 4)
    assert e.value.code == abi.PCC_E_STREAM
    assert GeometryCodec.lod_info(blob[:table_end], 4)[0] == need


# ------------------------------------------------------------------ GPU
def _coarse(points, k):
    """a Morton-ordered decode >> k with adjacent equal rows dropped"""
    c = np.asarray(points, np.int32) >> k
    if c.shape[0] == 0:
        return c
    keep = np.ones(c.shape[0], bool)
    keep[1:] = np.any(c[1:] != c[:-1], axis=1)
    return c[keep]


@pytest.mark.gpu
def test_mixed_batch_at_every_lod(wl):
    geo = pkg().GeometryCodec()
    frames = _mixed_frames(wl)
    blobs = geo.compress(frames)
    full = geo.decompress(blobs)
    for f, (a, b) in enumerate(zip(geo.decompress(blobs, lod=0), full)):
        assert np.array_equal(a, b), f
    for k in LODS:
        want = [_coarse(p, k) for p in full]
        for f, w in enumerate(want):
            assert w.shape[0] == _cells(frames[f], k).shape[0], (k, f)
        prefixes = [b[:geo.lod_info(b, k)[0]] for b in blobs]
        for what, src in (("whole blobs", blobs), ("exact prefixes", prefixes)):
            host = geo.decompress(src, lod=k)
            dev = geo.decompress(src, output="device", lod=k)
            assert len(host) == len(dev) == len(frames)
            for f, (w, h, d) in enumerate(zip(want, host, dev)):
                assert isinstance(h, np.ndarray) and h.dtype == np.int32 and h.shape == w.shape, (k, what, f, h.shape, w.shape)
                assert np.array_equal(h, w), f"lod {k}, {what}, frame {f}: host cells differ"
                assert d.is_cuda and np.array_equal(d.cpu().numpy(), w), f"lod {k}, {what}, frame {f}: device cells differ"
    geo.close()


def _pack(p):
    p = np.asarray(p, np.int64) + 32768
    return (p[:, 0] << 32) | (p[:, 1] << 16) | p[:, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 4])
def test_compress_at_a_lod_against_the_oracle(oracle, wl, k):
    geo = pkg().GeometryCodec()
    frames = _mixed_frames(wl)
    blobs = geo.compress(frames, lod=k)
    fine = geo.decompress(geo.compress(frames), lod=k)
    plain = geo.decompress(blobs)
    for f, p in enumerate(frames):
        ref = oracle.octree_encode(_cells(p, k), 32768 >> k, version=2)
        assert blobs[f] == ref, f"frame {f}: blob differs from the oracle's ({len(blobs[f])} vs {len(ref)} bytes)"
        assert np.array_equal(plain[f], fine[f]), f"frame {f}: cells differ from the fine blob's level {k}"
    # attributes: per cell and channel the rounded mean over ALL input rows of the cell
    rng = np.random.default_rng(5 + k)
    sweep = wl.lidar_sweep(seed=1)["points"]
    dup = frames[9]
    cases = [(sweep, wl.lidar_intensity(sweep, seed=1)),
             (frames[7], rng.integers(0, 65536, (frames[7].shape[0], 3)).astype(np.uint16)),
             (np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint16)),
             (dup, rng.integers(0, 65536, (dup.shape[0], 3)).astype(np.uint16))]
    gb, ab = geo.compress([p for p, _ in cases], attributes=[a for _, a in cases], lod=k)
    assert gb == geo.compress([p for p, _ in cases], lod=k)
    pts, got = geo.decompress(gb, ab)
    for f, (p, a) in enumerate(cases):
        a2 = a if a.ndim == 2 else a[:, None]
        u, mean = attr_ref.merge(np.asarray(p, np.int32) >> k, a2)
        assert pts[f].shape == u.shape, f
        idx = np.searchsorted(_pack(u), _pack(pts[f]))
        assert np.array_equal(u[idx], pts[f]), f
        assert got[f].dtype == a.dtype and np.array_equal(got[f], mean[idx]), f"frame {f}: merged values differ"
        assert ab[f] == attr_ref.encode(mean[idx], a.dtype.itemsize), f"frame {f}: attribute blob differs"
    geo.close()


def _batch8(oracle):
    rng = np.random.default_rng(188)
    return [oracle.octree_encode(_cloud(rng, int(n), extent=120), 32768, version=2)
            for n in (3000, 3500, 5000, 3200, 4500, 4000, 3600, 4800)]


@pytest.mark.gpu
def test_refusals_name_the_frame_and_the_ctx_stays_usable(rt, oracle, wl):
    abi = pkg("_abi")
    GeometryCodec = pkg().GeometryCodec
    blobs = _batch8(oracle)
    k5 = 5
    b5 = blobs[k5]
    d = b5[2]
    S, nc = struct.unpack_from("<2I", b5, 24 + 4 * d)
    level_n = struct.unpack_from(f"<{d}I", b5, 24)
    off_payload = 24 + 4 * d + 8 + 216 + 4 * nc
    assert nc == 1 and d >= 4
    assert (-(-sum(level_n[:d - 1]) // S) - 1) % 64 > 3                   # l* of lod 1 lies behind lane 3
    want = {k: [_coarse(oracle.octree_decode(b), k) for b in blobs] for k in (1, 2)}

    def with5(b):
        return blobs[:k5] + [bytes(b)] + blobs[k5 + 1:]

    def flipped(at, val):
        b = bytearray(b5)
        b[at] = val(b[at])
        return with5(b)

    sweep = oracle.octree_encode(_unique(wl.lidar_sweep(seed=1)["points"]), 32768, version=2)
    need = [GeometryCodec.lod_info(sweep, k)[0] for k in range(7)]
    assert all(a > b for a, b in zip(need, need[1:])), need               # strictly decreasing on the sweep
    cases = [
        ("a prefix two bytes short", 1, with5(b5[:GeometryCodec.lod_info(b5, 1)[0] - 2])),
        ("the prefix of lod 2 decoded at lod 1", 1, with5(sweep[:need[2]])),
        ("level_n of a level above the cut", 2, flipped(24 + 4 * 2, lambda v: v ^ 0x04)),
        ("len[3] of the last needed chunk", 1, flipped(off_payload + 256 + 2 * 3, lambda v: (v + 1) & 0xFF)),
    ]
    for what, k, batch in cases:
        with pytest.raises(abi.PccError) as e:
            rt.octree_decode_frames(batch, lod=k)
        assert e.value.code == abi.PCC_E_STREAM, what
        assert f"frame {k5}:" in str(e.value), (what, str(e.value))
        if "prefix" in what:
            assert "truncated" in str(e.value), (what, str(e.value))
        got = rt.octree_decode_frames(blobs, lod=k)                        # the next call on the same ctx
        assert all(np.array_equal(g, w) for g, w in zip(got, want[k])), what
    for bad in (16, -1):
        with pytest.raises(abi.PccError) as e:
            rt.octree_decode_frames(blobs, lod=bad)
        assert e.value.code == abi.PCC_E_ARG
    assert all(np.array_equal(g, w) for g, w in zip(rt.octree_decode_frames(blobs, lod=2), want[2]))
    geo = GeometryCodec()
    pts = [_cloud(np.random.default_rng(1), 500)]
    gb, ab = geo.compress(pts, attributes=[np.arange(500, dtype=np.uint8)])
    with pytest.raises(ValueError, match="attribute"):
        geo.decompress(gb, ab, lod=1)
    for bad in (16, -1):
        with pytest.raises(ValueError):
            geo.decompress(gb, lod=bad)
        with pytest.raises(ValueError):
            geo.compress(pts, lod=bad)
    assert geo.decompress(gb, lod=1)[0].shape[0] == _cells(pts[0], 1).shape[0]
    geo.close()


@pytest.mark.gpu
def test_two_codecs_at_two_lods_on_two_threads(wl):
    GeometryCodec = pkg().GeometryCodec
    rng = np.random.default_rng(2)
    seqs = [[wl.lidar_sweep(32, 900, seed=s)["points"] for s in range(4)] + [_cloud(rng, 9000)],
            [_cloud(rng, int(n), extent=150) for n in (70000, 10, 3000)] + [wl.lidar_sweep(seed=7)["points"]]]
    lods = (1, 3)
    one = GeometryCodec()
    blobs = [one.compress(s) for s in seqs]
    serial = [one.decompress(b, lod=k) for b, k in zip(blobs, lods)]
    serial_c = [one.compress(s, lod=k) for s, k in zip(seqs, lods)]
    codecs = [GeometryCodec(), GeometryCodec()]
    got = [None, None]
    errors = []

    def run(i):
        try:
            for _ in range(3):
                c = codecs[i].compress(seqs[i], lod=lods[i])
                pre = [b[:GeometryCodec.lod_info(b, lods[i])[0]] for b in blobs[i]]
                p = codecs[i].decompress(pre, lod=lods[i])
            got[i] = (c, p)
        except Exception as exc:           # surfaced below
            errors.append(exc)
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert got[i][0] == serial_c[i]
        assert all(np.array_equal(a, b) for a, b in zip(got[i][1], serial[i]))
    for c in codecs + [one]:
        c.close()
