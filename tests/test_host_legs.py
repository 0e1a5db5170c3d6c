"""The host legs of a GOP step: the decoded cloud's way to host memory (one tail kernel, points as int16
triples over the link, widened by the codec's threads), the points' upload piece by piece, and the z string's coder
tables kept per codec.  Every check compares with a path those changes do not touch, value for value: all of them are
integers or the result of the same three IEEE operations."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SETTINGS = [[1.0, 0.0], [0.0, 1.0], [1, 1]]
CORNER_SEED = 0   # see corner_frame


def corner_frame(seed):
    """points in the two outermost corners of the int16 lattice, (-32768,)*3 and (32767,)*3 among them: two seeded
    blobs of 32^3 cells.  The seed is chosen (with the CPU oracle alone) so that the oracle's lossy reconstruction
    still reaches the outermost latent cells on both sides; the test asserts that of the oracle's output."""
    rng = np.random.default_rng(seed)
    g = np.arange(32)
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lo = v[rng.random(v.shape[0]) < 0.35]
    hi = v[rng.random(v.shape[0]) < 0.35]
    pts = np.concatenate([[[0, 0, 0]], lo, [[65535, 65535, 65535]], 65535 - hi], 0).astype(np.int64) - 32768
    pts = np.unique(pts, axis=0)
    return {"points": pts.astype(np.int16), "colors": rng.random((pts.shape[0], 3))}


def _zed5():
    with np.load(os.path.join(GOLDEN, "zed_seq25.npz")) as f:
        return [{"points": f[f"points_{i}"], "colors": f[f"colors_u8_{i}"].astype(np.float64) / 255.0} for i in range(5)]


@pytest.fixture(scope="module")
def codec():
    c = pkg("native").NativeCodec(pkg("model").load_checkpoint("demo_small"), 0)
    yield c
    c.close()


def _encode_host(codec, frames, settings=SETTINGS):
    out, _, _ = codec.encode_host_frames([np.ascontiguousarray(f["points"]) for f in frames],
                                         [np.ascontiguousarray(f["colors"]) for f in frames], settings)
    return out


def _device_path(codec, data):
    """decode() -> device tensors -> .cpu() -> pack_batches' expression in numpy"""
    c4, col, offs, _, _ = codec.decode(data)
    pts = np.ascontiguousarray(c4.cpu().numpy()[:, 1:])
    cols = np.clip(np.nan_to_num(col.cpu().numpy(), nan=0.0) * np.float32(255), 0, 255) / np.float32(255)
    assert pts.dtype == np.int32 and cols.dtype == np.float32
    return pts, cols, offs


def _packed_raw(codec, data, extra=0, sentinel=-7):
    """pcc_decode_gop_packed into arrays of `extra` rows more than the container announces, prefilled"""
    abi = pkg("_abi")
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    cap = C.c_int64(0)
    abi.check(codec.lib.pcc_container_points(buf, len(data), C.byref(cap), None), "pcc_container_points")
    rows = cap.value + extra
    pts = np.full((rows, 3), sentinel, np.int32)
    cols = np.full((rows, 3), sentinel, np.float32)
    info, ts = abi.PccCloudInfo(), (C.c_double * 6)()
    abi.check(codec.lib.pcc_decode_gop_packed(codec.handle, buf, len(data), C.c_void_p(pts.ctypes.data),
                                              C.c_void_p(cols.ctypes.data), rows, C.byref(info), ts), "pcc_decode_gop_packed")
    return pts, cols, int(info.n_points)


def _fetch_packed(codec, data):
    """pcc_decode_gop, then pcc_decode_fetch_packed: the two-call form"""
    abi = pkg("_abi")
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    info, ts = abi.PccCloudInfo(), (C.c_double * 6)()
    abi.check(codec.lib.pcc_decode_gop(codec.handle, buf, len(data), C.byref(info), ts), "pcc_decode_gop")
    n = int(info.n_points)
    pts, cols = np.full((n, 3), -7, np.int32), np.full((n, 3), -7, np.float32)
    abi.check(codec.lib.pcc_decode_fetch_packed(codec.handle, C.c_void_p(pts.ctypes.data), C.c_void_p(cols.ctypes.data)),
              "pcc_decode_fetch_packed")
    return pts, cols


def _check_packed(codec, data):
    pts, cols, offs, _, _ = codec.decode(data, packed_host=True)
    rp, rc, roffs = _device_path(codec, data)
    assert offs == roffs and pts.shape == rp.shape and pts.shape[0] > 0
    assert np.array_equal(pts, rp) and np.array_equal(cols, rc)
    return pts, cols


@pytest.mark.parametrize("case", ["room200k", "zed_gop5"])
def test_packed_decode_equals_device_path(wl, codec, case):
    frames = [wl.room(200_000, seed=5)] if case == "room200k" else _zed5()
    if case == "zed_gop5":
        assert min(int(f["points"].min()) for f in frames) < 0
    for data in _encode_host(codec, frames):
        pts, cols = _check_packed(codec, data)
        fp, fc = _fetch_packed(codec, data)                 # pcc_decode_fetch_packed after a plain pcc_decode_gop
        assert np.array_equal(fp, pts) and np.array_equal(fc, cols)


def test_packed_decode_at_the_ends_of_the_int16_range(oracle, codec):
    """coordinates -32768 and 32767 go in, and the reconstruction still holds coordinates of the outermost latent cells
    (<= -32761, >= 32760): the int16 triples on the link carry both ends of their range"""
    frame = corner_frame(CORNER_SEED)
    assert frame["points"].min() == -32768 and frame["points"].max() == 32767
    ref, _ = oracle.compress([frame], SETTINGS)
    orec = oracle.decompress(ref[3])[0]
    assert orec["points"].min() <= -32761 and orec["points"].max() >= 32760, "corner_frame: pick another CORNER_SEED"
    out = _encode_host(codec, [frame])
    assert out[2] == ref[3]
    pts, cols = _check_packed(codec, out[2])
    assert np.array_equal(pts, orec["points"]) and np.array_equal(cols, orec["colors"])
    assert pts.min() <= -32761 and pts.max() >= 32760


def test_packed_decode_leaves_rows_beyond_n_untouched(wl, codec):
    frames = [wl.sphere_shell(40, 15.0, seed=5, offset=(-300, 20, 7)), wl.sphere_shell(24, 9.1, seed=2)]
    data = _encode_host(codec, frames)[2]
    rp, rc, _ = _device_path(codec, data)
    pts, cols, n = _packed_raw(codec, data, extra=1000, sentinel=-7)
    assert n == rp.shape[0] and pts.shape[0] >= n + 1000
    assert np.array_equal(pts[:n], rp) and np.array_equal(cols[:n], rc)
    assert (pts[n:] == -7).all() and (cols[n:] == -7).all()


def test_packed_decode_reuses_its_staging(wl):
    """two decodes in a row on a fresh codec, the larger cloud first: the second goes through the staging buffer the
    first one sized"""
    c = pkg("native").NativeCodec(pkg("model").load_checkpoint("demo_small"), 0)
    try:
        big = _encode_host(c, [wl.room(200_000, seed=6)])[2]
        small = _encode_host(c, [wl.sphere_shell(24, 9.1, seed=2, offset=(5, -900, 33))])[2]
        got = [c.decode(d, packed_host=True)[:2] for d in (big, small)]
        for d, (pts, cols) in zip((big, small), got):
            rp, rc, _ = _device_path(c, d)
            assert np.array_equal(pts, rp) and np.array_equal(cols, rc)
    finally:
        c.close()


def _frames_exact(wl, sizes, seed=11):
    frames = [wl.room(n, seed=seed + i, offset=(-200 + 7 * i, -150, -100 - 3 * i)) for i, n in enumerate(sizes)]
    assert [f["points"].shape[0] for f in frames] == list(sizes)
    return frames


@pytest.mark.parametrize("sizes", [(1000,), (174762,), (174763,), (1_000_000,), (30_000, 174_763, 1_001)])
@pytest.mark.parametrize("pdt", [np.int16, np.int32])
def test_host_frames_encode_equals_device_frames(wl, codec, sizes, pdt):
    """6 B x 174762 lies just below one 1-MB upload piece, 174763 just above"""
    frames = _frames_exact(wl, sizes)
    pts = [np.ascontiguousarray(f["points"].astype(pdt)) for f in frames]
    cols = [np.ascontiguousarray(f["colors"]) for f in frames]
    host, kh, _ = codec.encode_host_frames(pts, cols, SETTINGS)
    dev, kd, _ = codec.encode_frames([torch.from_numpy(p).cuda() for p in pts], [torch.from_numpy(c).cuda() for c in cols],
                                     SETTINGS)
    assert len(host) == 3 and kh == kd
    for q in range(3):
        assert host[q] == dev[q], f"container {q + 1} differs"


def test_two_codecs_keep_their_own_z_tables(wl, tmp_path):
    """two codecs alive in one process whose checkpoints differ in their entropy_bottleneck tables (two hyper widths):
    each round-trips its own GOP to ITS oracle's bytes and reconstruction, call by call in turn"""
    from oracle.codec_ref import Oracle
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        mk = importlib.import_module("make_checkpoint")
    finally:
        sys.path.pop(0)
    native = pkg("native")
    settings = [[1.0, 0.0], [1, 1]]
    gops = [[wl.sphere_shell(40, 15.3, seed=3, offset=(-30, 12, -70)), wl.sphere_shell(24, 9.1, seed=4)],
            [wl.body(20000, seed=2)]]
    sides = []
    try:
        for i, cz in enumerate((32, 8)):
            t = mk.build(32, 32, cz)
            np.savez(tmp_path / f"ckpt{i}.npz", **t)
            sides.append((native.NativeCodec(t, 0), Oracle(ckpt=str(tmp_path / f"ckpt{i}.npz"), threads=4)))
        assert not np.array_equal(np.asarray(mk.build(32, 32, 32)["entropy_bottleneck.quantized_cdf"])[:8],
                                  np.asarray(mk.build(32, 32, 8)["entropy_bottleneck.quantized_cdf"]))
        refs = [o.compress(g, settings)[0] for (_, o), g in zip(sides, gops)]
        for _ in range(2):
            outs = [_encode_host(c, g, settings) for (c, _), g in zip(sides, gops)]   # codec 0, codec 1, ...
            for (c, o), out, ref in zip(sides, outs, refs):
                assert out[0] == ref[1] and out[1] == ref[2]
            for (c, o), out in zip(sides, outs):
                pts, cols, offs, _, _ = c.decode(out[1], packed_host=True)
                for i, fr in enumerate(o.decompress(out[1])):
                    assert np.array_equal(pts[offs[i]:offs[i + 1]], fr["points"])
                    assert np.array_equal(cols[offs[i]:offs[i + 1]], fr["colors"])
    finally:
        for c, _ in sides:
            c.close()
