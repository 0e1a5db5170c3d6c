"""The attribute decoders' ordinary-memory h_out (pcc_attr_decode_frames / pcc_attr_decode_frames_lod through the C
ABI): Runtime.attr_decode_frames hands the library a device pointer or a pinned array, so the path a caller's pageable
array takes — the values down into the staging, copied out behind the synchronisation — is run here alone.  Its bytes,
h_out_offsets and h_format must equal those of Runtime.attr_decode_frames(device=False) and (device=True) for the same
blobs, one case per decode body and side-table combination; a capacity one byte short is PCC_E_NOMEM and writes
nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg, random_cloud

FILL = 0xA5

# name -> (compress settings, decoded at these levels of detail; None: pcc_attr_decode_frames)
CASES = {
    "v1": (dict(), (None,)),
    "v13": (dict(max_error=2, cross_channel=True), (None,)),
    "v2": (dict(scalable=True), (0, 2)),
    "v14": (dict(scalable=True, max_error=2, cross_channel=True), (0, 2)),
    "v19": (dict(qstep=5), (0,)),
    "v21": (dict(qstep=(3, 9, 17, 6), colour="ycocg"), (0,)),
}
VERSION = {"v1": 1, "v13": 13, "v2": 2, "v14": 14, "v19": 19, "v21": 21}


@pytest.fixture(scope="module")
def geo():
    g = pkg().GeometryCodec()
    yield g
    g.close()


@pytest.fixture(scope="module")
def frames():
    """uint8 x 4 with 8193 distinct points (two chunks at c = 4), no points, one point, uint16 x 3 with 300 points"""
    rng = np.random.default_rng(77)
    pts = [random_cloud(rng, 8193, extent=96, lo=-20)[:, 1:].astype(np.int32), np.zeros((0, 3), np.int32),
           np.array([[3, -7, 11]], np.int32), random_cloud(rng, 300, extent=48, lo=-20)[:, 1:].astype(np.int32)]
    attrs = [rng.integers(0, 256, (8193, 4)).astype(np.uint8), np.zeros((0, 4), np.uint8),
             rng.integers(0, 256, (1, 4)).astype(np.uint8), rng.integers(0, 65536, (300, 3)).astype(np.uint16)]
    return pts, attrs


@pytest.fixture(scope="module")
def coded(geo, frames):
    """name -> (geometry blobs, attribute blobs) of the four frames, compressed once per kind"""
    made = {}

    def get(name):
        if name not in made:
            pts, attrs = frames
            kw = CASES[name][0]
            if name == "v21":      # a step per channel: the frames of four and of three channels in a call each
                g4, a4 = geo.compress(pts[:3], attributes=attrs[:3], **kw)
                g3, a3 = geo.compress(pts[3:], attributes=attrs[3:], **dict(kw, qstep=kw["qstep"][:3]))
                made[name] = (g4 + g3, a4 + a3)
            else:
                made[name] = geo.compress(pts, attributes=attrs, **kw)
            assert [b[1] for b in made[name][1]] == [VERSION[name]] * 4
        return made[name]
    return get


def _call(rt, blobs, lod, cells):
    """the entry point of Runtime.attr_decode_frames for these blobs, its output arguments left open, and the arrays it
    fills: call(d_out, h_out, cap_bytes), offs, fmt"""
    nb = len(blobs)
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
    ptrs = (C.c_void_p * nb)(*[b.ctypes.data for b in bufs])
    lens = (C.c_int64 * nb)(*[b.shape[0] for b in bufs])
    offs = (C.c_int64 * (nb + 1))()
    fmt = (C.c_int32 * nb)()
    if lod is None:
        call = lambda *a: rt.lib.pcc_attr_decode_frames(rt.ctx, ptrs, lens, nb, None, *a, offs, fmt)
    else:
        cell_offs = np.cumsum([0] + [int(c.shape[0]) for c in cells])
        coffs = (C.c_int64 * (nb + 1))(*[int(v) for v in cell_offs])
        base = C.c_void_p(next(c.data_ptr() - 12 * int(o) for c, o in zip(cells, cell_offs) if c.shape[0]))
        call = lambda *a: rt.lib.pcc_attr_decode_frames_lod(rt.ctx, ptrs, lens, nb, int(lod), base, coffs, *a, offs, fmt)
    call.keep = (bufs, ptrs, lens)
    return call, offs, fmt


def _decode(geo, gblobs, ablobs, lod):
    """-> (Runtime's arrays on the host, Runtime's device result copied to the host, the pageable buffer, offs, fmt,
    call)"""
    with geo._lock, geo.rt as rt:
        cells = None if lod is None else rt.octree_decode_frames(gblobs, device=True, lod=lod)
        kw = {} if lod is None else dict(lod=lod, cells=cells)
        host = rt.attr_decode_frames(ablobs, device=False, **kw)
        dev = [t.cpu().numpy() for t in rt.attr_decode_frames(ablobs, device=True, **kw)]
        call, offs, fmt = _call(rt, ablobs, lod, cells)
        assert call(None, None, 0) == 0
        total = offs[len(ablobs)]
        sized = (list(offs), list(fmt))
        out = np.empty(total + 32, np.uint8)      # ordinary memory: neither pinned nor the device's
        out[:] = FILL
        rc = call(None, C.c_void_p(out.ctypes.data), total)
        assert rc == 0, rt.lib.pcc_last_error()
        assert (list(offs), list(fmt)) == sized
        short = np.full(total + 32, FILL, np.uint8)
        rc_short = call(None, C.c_void_p(short.ctypes.data), total - 1)
    return host, dev, out, list(offs), list(fmt), (rc_short, short)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lod", [(n, k) for n, (_, lods) in CASES.items() for k in lods],
                         ids=[f"{n}-lod{k}" if k is not None else n for n, (_, lods) in CASES.items() for k in lods])
def test_pageable_h_out_equals_the_runtime_both_ways(geo, coded, name, lod):
    abi = pkg("_abi")
    gblobs, ablobs = coded(name)
    host, dev, out, offs, fmt, (rc_short, short) = _decode(geo, gblobs, ablobs, lod)
    assert len(host) == len(dev) == 4 and offs[0] == 0
    rows = [a.shape[0] for a in host]
    if not lod:
        assert rows == [8193, 0, 1, 300]
    else:
        assert 0 < rows[0] < 8193 and rows[1] == 0 and rows[2] == 1 and 0 < rows[3] <= 300
    at = 0
    for f, (h, d) in enumerate(zip(host, dev)):
        assert h.dtype == d.dtype and h.shape == d.shape and np.array_equal(h, d), f
        assert fmt[f] == (h.dtype.itemsize | (h.shape[1] << 8)), f                      # h_format, from what Runtime made of it
        assert offs[f] == at, f                                                          # h_out_offsets: every frame on 16 bytes
        if h.size and host[0].size:                                                      # .. and where Runtime's views lie
            assert offs[f] == h.ctypes.data - host[0].ctypes.data, f
        got = out[offs[f]:offs[f] + h.nbytes].view(h.dtype).reshape(h.shape)
        assert np.array_equal(got, h), f"frame {f}: the pageable array differs from Runtime's"
        at = (at + h.nbytes + 15) // 16 * 16
    assert offs[4] == at
    assert np.all(out[offs[4]:] == FILL)                                                 # nothing behind the call's bytes
    # a capacity one byte short: refused before anything is written
    assert rc_short == abi.PCC_E_NOMEM
    assert np.all(short == FILL)
