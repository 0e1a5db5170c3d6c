"""The attribute lane decoder (k_a_dec in csrc/attr.hip, behind every attribute blob kind) and the kernels that index by
the header's S behind it (k_a4_recon, k_a8_recon, k_ax_inv, k_a2_walk), on what the parsers accept and
GeometryCodec.compress never writes: foreign layouts and fills of the last chunk, initial tables at the bounds, chunks
on both sides of the room for a chunk's words in LDS (alone and in one call), streams damaged so that the status is
known in advance, and every call's bytes inside its output.  Blobs come from the numpy restatements with layout= and
p0= (attr_layout_cases.py; tests/test_attr_layouts.py checks the same blobs on the host).  Every comparison is exact.

The two word routes.  k_a_dec copies a chunk's words to LDS when avail <= lds_words, and else reads them where they lie
in HBM; lds_words = min(cw_max, room), room = (131072 - 128 (nctx_max + 1)) / 2 = 65472 - 5120 c bpv 16-bit words for
the widest (bpv, c) of the CALL: 24 512 for four uint16 channels, 34 752 for three (attr_layout_cases.ROOMS).  The
words per chunk the restatement produced for the frames below (asserted from the blobs' own chunk tables):
    big, 8192 x 4 random uint16, one chunk                        CW_BIG          above 24 512
    big as version 2, the last chunk's words in the prefix of     lod 0, 1: above; lod 2: below      (LAST_WORDS_BIG2)
    300 x 1 uint8 and 2400 x 4 uint16, beside big in one call     both below 24 512
    16384 x 4 uint16, 8192 random and 8192 constant points        CW_HALVES, one chunk on each side, in either order"""
import ctypes as C
import re
import struct

import numpy as np
import pytest

import attr2_ref
import attr_cross_ref
import attr_layout_cases as K
import attr_nl_ref
import attr_ref
from conftest import pkg, random_cloud

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0xA5
ROOM4 = 24512                          # K.room(2, 4)
CW_BIG = 33858
LAST_WORDS_BIG2 = {0: 33856, 1: 30698, 2: 16502}
CW_HALVES = (33980, 320)               # the random half, the constant half


@pytest.fixture(scope="module")
def geo(rt):
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _np(arrays):
    return [a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in arrays]


def _decode1(rt, blobs, device):
    return _np(rt.attr_decode_frames(blobs, device=device))


def _decode2(rt, gblobs, blobs, lod, device):
    cells = rt.octree_decode_frames(gblobs, device=True, lod=lod)
    return _np(rt.attr_decode_frames(blobs, device=device, lod=lod, cells=cells))


def _same(got, want, ids):
    assert len(got) == len(want)
    for g, w, i in zip(got, want, ids):
        assert g.dtype in (np.uint8, np.uint16), i
        assert g.shape == w.shape and np.array_equal(g.astype(np.int64), w), i


def _raw(rt, blobs, lod=None, cells=None):
    """the entry point Runtime.attr_decode_frames calls for these blobs, straight into the middle of a device tensor
    filled with FILL that is 64 bytes longer than the call's bytes at each end -> (the tensor on the host, offs, fmt)"""
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
    assert call(None, None, 0) == 0, rt.lib.pcc_last_error()
    total = offs[nb]
    out = torch.full((total + 128,), FILL, dtype=torch.uint8, device=rt.device)
    rt.sync()
    assert call(C.c_void_p(out.data_ptr() + 64), None, total) == 0, rt.lib.pcc_last_error()
    rt.sync()
    return out.cpu().numpy(), list(offs), list(fmt)


def _inside(raw, want, ids):
    """the frames' values at their 16-byte-aligned places; the guard bytes and the padding between frames untouched"""
    out, offs, fmt = raw
    used = np.zeros(out.shape[0], bool)
    for f, (w, i) in enumerate(zip(want, ids)):
        bpv, c = fmt[f] & 0xFF, fmt[f] >> 8
        assert offs[f] % 16 == 0 and c == w.shape[1], i
        lo, hi = 64 + offs[f], 64 + offs[f] + w.size * bpv
        assert hi <= 64 + offs[f + 1], i
        got = out[lo:hi].view(np.uint8 if bpv == 1 else np.uint16).reshape(w.shape)
        assert np.array_equal(got.astype(np.int64), w), i
        used[lo:hi] = True
    assert out.shape[0] == offs[len(want)] + 128
    assert (out[~used] == FILL).all(), "bytes outside the frames' values were written"
    assert (~used[:64]).all() and (~used[-64:]).all()


# ------------------------------------------------------------------------------------------ a. layouts, b. tables
@pytest.fixture(scope="module")
def sweep(geo):
    """the frames of K.sweep_cases() and K.table_cases(): ids, version-1 blobs and values, version-2 blobs with the
    geometry blobs of their points and the points and values in Morton order"""
    cases = [(i, p, v, bpv, dict(layout=lay)) for i, p, v, bpv, lay in K.sweep_cases()]
    cases += [(i, p, v, bpv, dict(p0=p0)) for i, p, v, bpv, p0 in K.table_cases()]
    ids = [c[0] for c in cases]
    b1 = [attr_ref.encode(v, bpv, **kw) for _, _, v, bpv, kw in cases]
    b2 = [attr2_ref.encode(p, v, bpv, **kw) for _, p, v, bpv, kw in cases]
    mort = [K.morton(p, v) for _, p, v, _, _ in cases]
    gblobs = geo.compress([p for _, p, _, _, _ in cases])
    for (_, _, v, bpv, kw), x, y in zip(cases, b1, b2):      # the blobs are what the case says
        for b in (x, y):
            _, n, S, nc, p0, words, _, _ = K.head_of(b)
            assert n == v.shape[0] and (S, nc) == kw.get("layout", attr_ref.layout(*v.shape))
            assert "p0" not in kw or np.array_equal(p0, kw["p0"])
            assert max(words) <= K.room(bpv, v.shape[1])          # every chunk of these goes through LDS
    return ids, b1, [v for _, _, v, _, _ in cases], b2, gblobs, mort


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_version_1_layouts_and_tables(rt, sweep, device):
    ids, b1, vals, _, _, _ = sweep
    assert len({K.head_of(b)[2:4] for b in b1}) >= 12            # one call, many layouts
    _same(_decode1(rt, b1, device), vals, ids)
    for i, b, v in zip(ids, b1, vals):                           # and each alone
        _same(_decode1(rt, [b], device), [v], [i])


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("lod", [0, 1, 3])
def test_version_2_layouts_and_tables(rt, sweep, lod, device):
    ids, _, _, b2, gblobs, mort = sweep
    want = [K.sample(ps, vs, lod)[1] if lod else vs for ps, vs in mort]
    info = [attr2_ref.lod_info(b, lod, any_layout=True) for b in b2]
    assert [m for _, m in info] == [w.shape[0] for w in want]
    if lod:                                                      # prefixes that end inside their last chunk
        assert sum(nbytes < len(b) for (nbytes, _), b in zip(info, b2)) >= len(b2) // 2
    prefixes = [b[:nbytes] for (nbytes, _), b in zip(info, b2)]
    _same(_decode2(rt, gblobs, prefixes, lod, device), want, ids)
    if device:
        pick = [k for k in range(len(ids)) if k % 4 == lod % 4]   # some alone
        for k in pick:
            _same(_decode2(rt, [gblobs[k]], [prefixes[k]], lod, device), [want[k]], [ids[k]])


OUTSIDE = [("S c = 513", 1000, 1, (512, 1), (513, 1)), ("S c = 516", 1000, 4, (128, 1), (129, 1)), ("64 S nc = n - 1", 961, 3, (3, 6), (3, 5)),
           ("64 S (nc - 1) = n", 960, 3, (3, 5), (3, 6)), ("nc = n + 1", 1, 3, (1, 1), (1, 2))]


def test_version_1_layouts_one_step_outside_are_refused(rt):
    """version 1's S is read by no host-only entry point: pcc_attr_decode_frames refuses it before anything is launched"""
    abi = pkg("_abi")
    good = attr_ref.encode(K.values(300, 1, 1, 3), 1)
    for what, n, c, lay, bad in OUTSIDE:
        for e in (0, 2):
            vals = K.values(n, c, 1, 11)
            blob = bytearray(attr_nl_ref.encode(vals, 1, e, layout=lay))
            at = attr_ref.HEAD + (4 if e else 0)
            assert struct.unpack_from("<II", blob, at) == lay
            struct.pack_into("<II", blob, at, *bad)
            with pytest.raises(abi.PccError) as err:
                rt.attr_decode_frames([good, bytes(blob)] if e == 0 else [bytes(blob)])
            assert err.value.code == abi.PCC_E_STREAM, what
            assert "frame %d:" % (1 if e == 0 else 0) in str(err.value) and "%d points in %d chunks of 64 x %d" % (n, bad[1], bad[0]) in str(err.value)
    assert np.array_equal(_decode1(rt, [good], True)[0], K.values(300, 1, 1, 3))


# ------------------------------------------------------------------------------------------ c. the two word routes
@pytest.fixture(scope="module")
def heavy(geo):
    """big and the frames around it, built once"""
    rng = np.random.default_rng(2024)
    pts = random_cloud(rng, 8192, extent=64, lo=-30)[:, 1:].astype(np.int32)
    vals = rng.integers(0, 65536, (8192, 4))
    ps, vs = K.morton(pts, vals)
    h = dict(pts=pts, vals=vals, ps=ps, vs=vs)
    h["b1"] = attr_ref.encode(vs, 2)
    h["b2"] = attr2_ref.encode(pts, vals, 2)
    h["small"] = K.values(300, 1, 1, 1)
    h["small_pts"] = K.points(300, 1)
    h["wide"] = rng.integers(0, 65536, (2400, 4))
    h["wide_pts"] = K.points(2400, 2)
    h["small1"], h["wide1"] = attr_ref.encode(h["small"], 1), attr_ref.encode(h["wide"], 2)
    const = np.tile(np.array([[7, 65535, 0, 31000]]), (8192, 1))
    h["halves"] = [np.concatenate([vs, const]), np.concatenate([const, vs])]
    h["halves1"] = [attr_ref.encode(v, 2) for v in h["halves"]]
    h["gblobs"] = geo.compress([h["small_pts"], pts, h["wide_pts"]])
    return h


def _words(blob):
    return K.head_of(blob)[5]


def test_which_side_of_the_room_every_heavy_chunk_falls(heavy):
    """the figures of this file's docstring, from the blobs' own chunk tables"""
    assert K.room(2, 4) == ROOM4 == K.ROOMS[(2, 4)]
    assert K.head_of(heavy["b1"])[2:4] == (128, 1) and _words(heavy["b1"]) == [CW_BIG] and CW_BIG > ROOM4
    assert len(_words(heavy["small1"])) == 1 and _words(heavy["small1"])[0] <= ROOM4
    assert len(_words(heavy["wide1"])) == 1 and 192 + 2400 * 4 // 2 < _words(heavy["wide1"])[0] <= ROOM4
    assert K.head_of(heavy["small1"])[4].shape[0] == 80 and K.head_of(heavy["wide1"])[4].shape[0] == 640
    assert [_words(b) for b in heavy["halves1"]] == [list(CW_HALVES), list(CW_HALVES)[::-1]]
    assert CW_HALVES[0] > ROOM4 >= CW_HALVES[1]
    _, _, _, nc, _, words, _, off_payload = K.head_of(heavy["b2"])
    assert nc == 1
    last = {k: (attr2_ref.lod_info(heavy["b2"], k)[0] - off_payload) // 2 for k in (0, 1, 2)}
    assert last == LAST_WORDS_BIG2 and last[0] == words[0]
    assert last[0] > ROOM4 and last[1] > ROOM4 and last[2] <= ROOM4


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_a_chunk_above_the_room_alone_and_between_lighter_frames(rt, heavy, device):
    assert _words(heavy["b1"])[0] > ROOM4
    _same(_decode1(rt, [heavy["b1"]], device), [heavy["vs"]], ["big alone"])
    # one call: both routes, nctx 80, 640 and 640 with big's words behind 641 model rows
    blobs = [heavy["small1"], heavy["b1"], heavy["wide1"]]
    assert [_words(b)[0] > ROOM4 for b in blobs] == [False, True, False]
    _same(_decode1(rt, blobs, device), [heavy["small"], heavy["vs"], heavy["wide"]], ["300x1", "big", "2400x4"])
    # a narrower frame beside it does not widen the room of the call: nctx_max stays big's
    _same(_decode1(rt, [heavy["b1"], heavy["small1"]], device), [heavy["vs"], heavy["small"]], ["big", "300x1"])


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_one_frame_with_a_chunk_on_each_side_of_the_room(rt, heavy, device):
    for blob, vals, i in zip(heavy["halves1"], heavy["halves"], ("random | constant", "constant | random")):
        w = _words(blob)
        assert len(w) == 2 and min(w) <= ROOM4 < max(w)
        _same(_decode1(rt, [blob], device), [vals], [i])
    _same(_decode1(rt, heavy["halves1"], device), heavy["halves"], ["random | constant", "constant | random"])


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("lod", [0, 1, 2])
def test_big_as_version_2_on_either_side_of_the_room(rt, heavy, lod, device):
    nbytes, m = attr2_ref.lod_info(heavy["b2"], lod)
    last = (nbytes - K.head_of(heavy["b2"])[7]) // 2
    assert (last > ROOM4) == (lod < 2)
    want = K.sample(heavy["ps"], heavy["vs"], lod)[1] if lod else heavy["vs"]
    assert want.shape[0] == m
    _same(_decode2(rt, heavy["gblobs"][1:2], [heavy["b2"][:nbytes]], lod, device), [want], ["big v2"])
    if lod == 1:                                                 # between two lighter frames: both routes in one call
        sides = [attr2_ref.encode(heavy["small_pts"], heavy["small"], 1), attr2_ref.encode(heavy["wide_pts"], heavy["wide"], 2)]
        blobs = [sides[0], heavy["b2"], sides[1]]
        cut = [b[:attr2_ref.lod_info(b, 1)[0]] for b in blobs]
        wants = [K.sample(*K.morton(heavy["small_pts"], heavy["small"]), 1)[1], want, K.sample(*K.morton(heavy["wide_pts"], heavy["wide"]), 1)[1]]
        _same(_decode2(rt, heavy["gblobs"], cut, 1, device), wants, ["300x1", "big", "2400x4"])


def test_the_encoder_at_a_chunk_above_the_room(geo, heavy):
    _, ablobs = geo.compress([heavy["pts"]], attributes=[heavy["vals"].astype(np.uint16)])
    assert ablobs[0] == heavy["b1"]
    _, ablobs = geo.compress([heavy["pts"]], attributes=[heavy["vals"].astype(np.uint16)], scalable=True)
    assert ablobs[0] == heavy["b2"]


# ------------------------------------------------------------------------------------------ d. kinds that index by S
def test_kinds_behind_the_lane_decoder_off_the_encoders_layout(rt, geo):
    """k_a4_recon (version 4), k_ax_inv and k_a8_recon (version 8, every channel in the mask), k_a2_walk behind
    k_a_dec<true> (versions 7 and 11 at lod 0 and 2)"""
    frames = {name: K.frame(name) for name in K.FRAMES}
    frames["1000x4 uint8"] = K.frame((1000, 4, 1))
    lays = {"1000x3 uint8": ((3, 6), (170, 1)), "700x2 uint16": ((8, 2), (256, 1)), "1000x4 uint8": ((1, 16), (128, 1))}
    v4, want4, v8, want8, ids = [], [], [], [], []
    for name, (pts, vals, bpv) in frames.items():
        for lay in lays[name]:
            assert lay != attr_ref.layout(*vals.shape)
            ids.append("%s %s" % (name, lay))
            v4.append(attr_nl_ref.encode(vals, bpv, 2, layout=lay))
            want4.append(attr_nl_ref.decode(v4[-1], any_layout=True)[0])
            assert np.abs(want4[-1] - vals).max() == 2 and K.head_of(v4[-1])[2:4] == lay
            v8.append(attr_cross_ref.encode(vals, bpv, True, layout=lay))
            want8.append(vals)
            assert v8[-1][1] == 8 and v8[-1][3] >> 4 == (1 << (vals.shape[1] - 1)) - 1 and K.head_of(v8[-1])[2:4] == lay
    assert any(K.head_of(b)[2] * (b[3] & 15) == 512 for b in v4)
    for device in (True, False):
        _same(_decode1(rt, v4, device), want4, ids)
        _same(_decode1(rt, v8, device), want8, ids)
    pts, vals, bpv = frames["1000x3 uint8"]
    ps, vs = K.morton(pts, vals)
    gblobs = geo.compress([pts])
    b7 = attr_nl_ref.encode(vals, bpv, 2, points=pts, layout=(3, 6))
    b11 = attr_cross_ref.encode(vals, bpv, True, points=pts, layout=(170, 1))
    for lod in (0, 2):
        cells, first = K.sample(ps, vs, lod)
        n7, n11 = attr_nl_ref.lod_info(b7, lod, any_layout=True)[0], attr_cross_ref.lod_info(b11, lod, any_layout=True)[0]
        want7 = attr_nl_ref.decode(b7[:n7], cells, lod, any_layout=True)[0]
        assert np.abs(want7 - first).max() <= 2
        for device in (True, False):
            _same(_decode2(rt, gblobs, [b7[:n7]], lod, device), [want7], ["v7 (3, 6) lod %d" % lod])
            _same(_decode2(rt, gblobs, [b11[:n11]], lod, device), [first], ["v11 (170, 1) lod %d" % lod])


# ------------------------------------------------------------------------------------------ e. constructed bad streams
def _status(err):
    return int(re.search(r"status (\d+)", str(err)).group(1))


@pytest.fixture(scope="module")
def light(geo):
    """the frame of the LDS route, 1000 x 3 uint8 at (8, 2): every lane of chunk 0 holds 8 points; and the frames around it"""
    pts, vals, bpv = K.frame("1000x3 uint8")
    ps, vs = K.morton(pts, vals)
    side = [K.frame((300, 1, 1)), K.frame((700, 2, 2))]
    f = dict(vals=vals, vs=vs, b1=attr_ref.encode(vals, bpv, layout=(8, 2)), b2=attr2_ref.encode(pts, vals, bpv, layout=(8, 2)))
    f["side1"] = [attr_ref.encode(v, b) for _, v, b in side]
    f["side2"] = [attr2_ref.encode(p, v, b) for p, v, b in side]
    f["side_vals"] = [v for _, v, _ in side]
    f["side_vs"] = [K.morton(p, v)[1] for p, v, _ in side]
    f["gblobs"] = geo.compress([side[0][0], pts, side[1][0]])
    assert max(K.head_of(f["b1"])[5]) <= K.room(2, 2) and max(K.head_of(f["b2"])[5]) <= K.room(2, 2)
    return f


def _refused(rt, call, want_status):
    abi = pkg("_abi")
    with pytest.raises(abi.PccError) as err:
        call()
    assert err.value.code == abi.PCC_E_STREAM, str(err.value)
    assert "frame 1:" in str(err.value) and "corrupt stream" in str(err.value), str(err.value)
    assert want_status != 0 and _status(err.value) == want_status, str(err.value)


@pytest.mark.parametrize("how", K.DAMAGE)
def test_constructed_bad_streams_through_lds(rt, light, how):
    bad = K.damage(light["b1"], how)
    assert bad != light["b1"] and len(bad) - len(light["b1"]) == {"table entry + 1": 2, "table entry - 1": -2}.get(how, 0)
    want = attr_ref.status(bad)
    good = [light["side1"][0], light["b1"], light["side1"][1]]
    good_vals = [light["side_vals"][0], light["vals"], light["side_vals"][1]]
    for device in (True, False):
        _refused(rt, lambda: rt.attr_decode_frames([good[0], bad, good[2]], device=device), want)
        _same(_decode1(rt, good, device), good_vals, "012")
    # version 2, whole at lod 0 and as the prefix of lod 1 (the table entry belongs to a chunk that level does not need)
    bad2 = K.damage(light["b2"], how)
    good2 = [light["side2"][0], light["b2"], light["side2"][1]]
    for lod in (0, 1):
        if lod and how.startswith("table"):
            continue
        cut = lambda b: b[:attr2_ref.lod_info(b, lod, any_layout=True)[0]]
        m = attr2_ref.lod_info(bad2, lod, any_layout=True)[1]
        want = attr2_ref.status(cut(bad2), m, any_layout=True, whole=lod == 0)
        cells = rt.octree_decode_frames(light["gblobs"], device=True, lod=lod)
        _refused(rt, lambda: rt.attr_decode_frames([cut(good2[0]), cut(bad2), cut(good2[2])], device=True, lod=lod, cells=cells), want)
        got = _np(rt.attr_decode_frames([cut(b) for b in good2], device=True, lod=lod, cells=cells))
        if lod == 0:
            _same(got, [light["side_vs"][0], light["vs"], light["side_vs"][1]], "012")


@pytest.mark.parametrize("how", K.DAMAGE)
def test_constructed_bad_streams_read_in_place(rt, heavy, how):
    bad = K.damage(heavy["b1"], how)
    assert K.head_of(bad)[5][0] > ROOM4
    want = attr_ref.status(bad)
    good = [heavy["small1"], heavy["b1"], heavy["wide1"]]
    device = how in K.DAMAGE[::2]
    _refused(rt, lambda: rt.attr_decode_frames([good[0], bad, good[2]], device=device), want)
    _same(_decode1(rt, good, device), [heavy["small"], heavy["vs"], heavy["wide"]], "012")


# ------------------------------------------------------------------------------------------ f. inside its output
def test_every_call_stays_inside_its_output(rt, sweep, heavy):
    ids, b1, vals, b2, gblobs, mort = sweep
    _inside(_raw(rt, b1), vals, ids)
    for lod in (0, 1, 3):
        cells = rt.octree_decode_frames(gblobs, device=True, lod=lod)
        want = [K.sample(ps, vs, lod)[1] if lod else vs for ps, vs in mort]
        cut = [b[:attr2_ref.lod_info(b, lod, any_layout=True)[0]] for b in b2]
        _inside(_raw(rt, cut, lod, cells), want, ids)
    _inside(_raw(rt, [heavy["b1"]]), [heavy["vs"]], ["big"])
    _inside(_raw(rt, [heavy["small1"], heavy["b1"], heavy["wide1"]]), [heavy["small"], heavy["vs"], heavy["wide"]], "012")
    _inside(_raw(rt, heavy["halves1"]), heavy["halves"], "01")
    for lod in (0, 1, 2):
        cells = rt.octree_decode_frames(heavy["gblobs"][1:2], device=True, lod=lod)
        want = K.sample(heavy["ps"], heavy["vs"], lod)[1] if lod else heavy["vs"]
        _inside(_raw(rt, [heavy["b2"][:attr2_ref.lod_info(heavy["b2"], lod)[0]]], lod, cells), [want], ["big v2"])
