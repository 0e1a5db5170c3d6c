"""Attribute blobs off the encoder's layout and table, on the host.  The parsers of csrc/attr_blob.h take any
(S, n_chunks) with S >= 1, S c <= 512, 1 <= n_chunks <= n and 64 S (n_chunks - 1) < n <= 64 S n_chunks, and any initial
table in [16, 4080]; GeometryCodec.compress writes one layout per (n, c) and the table it counted.  Here the numpy
restatements write the others (attr_layout_cases.py lists them; tests/test_gpu_attr_decoder_edges.py decodes the same
blobs on the GPU), read them back, and the host-only entry points pcc_attr_info and pcc_attr_lod_info must say about
them what the restatements say; a layout one step outside each condition is PCC_E_STREAM.

Version 1 and its kin (4, 8, 13) have no host-only entry point that reads S: pcc_attr_info stops at the head.  Their
refusals are in the GPU file, at pcc_attr_decode_frames."""
import struct

import numpy as np
import pytest

import attr2_ref
import attr_cross_ref
import attr_layout_cases as K
import attr_nl_ref
import attr_ref
from conftest import pkg

SWEEP = K.sweep_cases()
TABLES = K.table_cases()


def test_rooms_and_layouts_are_what_the_files_say():
    for (bpv, c), want in K.ROOMS.items():
        assert K.room(bpv, c) == want == 65472 - 5120 * c * bpv
    assert K.sweep_layouts(1000, 3) == [(16, 1), (1, 16), (3, 6), (8, 2), (170, 1)]
    assert K.sweep_layouts(700, 2) == [(11, 1), (1, 11), (3, 4), (8, 2), (256, 1)]
    for _, _, vals, _, lay in SWEEP:
        attr_ref.check_layout(vals.shape[0], vals.shape[1], *lay)
    for bad in ((1000, 3, 171, 1), (1000, 3, 0, 1), (961, 3, 3, 5), (960, 3, 3, 6), (1, 1, 1, 2), (5, 1, 1, 0)):
        with pytest.raises(AssertionError):
            attr_ref.check_layout(*bad)
    with pytest.raises(AssertionError):
        attr_ref.encode(np.zeros((10, 1), np.int64), 1, p0=15)
    with pytest.raises(AssertionError):
        attr_ref.encode(np.zeros((10, 1), np.int64), 1, p0=[4081] * 80)


def _check_empty_lanes(blob, n):
    """lanes without points: no words, and the state the encoder starts from"""
    _, _, S, nc, _, words, _, off_payload = K.head_of(blob)
    for k in range(nc):
        x, ln = K.chunk_lanes(blob, off_payload, words, k)
        none = (k * 64 + np.arange(64)) * S >= n
        assert (ln[none] == 0).all() and (x[none] == 1 << 16).all()
        assert 192 + ln.sum() == words[k]
    return S, nc


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_reference_round_trips_and_the_host_entry_points_agree(case):
    _, pts, vals, bpv, lay = case
    Runtime = pkg("runtime").Runtime
    n, c = vals.shape
    b1 = attr_ref.encode(vals, bpv, layout=lay)
    assert _check_empty_lanes(b1, n) == lay
    got, b = attr_ref.decode(b1)
    assert b == bpv and np.array_equal(got, vals) and attr_ref.status(b1) == 0
    assert Runtime.attr_info(b1) == attr_nl_ref.info(b1)
    b2 = attr2_ref.encode(pts, vals, bpv, layout=lay)
    assert _check_empty_lanes(b2, n) == lay
    ps, vs = K.morton(pts, vals)
    got, b = attr2_ref.decode(b2, pts, any_layout=True)
    assert b == bpv and np.array_equal(got, vs)
    assert Runtime.attr_info(b2) == attr_nl_ref.info(b2)
    if lay != attr_ref.layout(n, c):                                      # the default path still insists on the encoder's
        with pytest.raises(AssertionError):
            attr2_ref.lod_info(b2, 0)
        with pytest.raises(AssertionError):
            attr2_ref.decode(b2, pts)
    prev = len(b2)
    for k in range(16):
        want = attr2_ref.lod_info(b2, k, any_layout=True)
        assert Runtime.attr_lod_info(b2, k) == want, k
        assert Runtime.attr_lod_info(b2[:prev], k) == want, k            # from the next finer level's prefix
        assert want[0] <= prev and want[1] == K.sample(ps, vs, k)[0].shape[0]
        prev = want[0]
        assert attr2_ref.status(b2[:want[0]], want[1], any_layout=True) == 0
    for k in (1, 3):                                                      # the levels the GPU file decodes
        cells, want = K.sample(ps, vs, k)
        nbytes = attr2_ref.lod_info(b2, k, any_layout=True)[0]
        assert np.array_equal(attr2_ref.decode(b2[:nbytes], cells, k, any_layout=True)[0], want)


@pytest.mark.parametrize("case", TABLES, ids=[c[0] for c in TABLES])
def test_tables_round_trip_and_the_host_entry_points_agree(case):
    _, pts, vals, bpv, p0 = case
    Runtime = pkg("runtime").Runtime
    b1 = attr_ref.encode(vals, bpv, p0=p0)
    assert np.array_equal(K.head_of(b1)[4], p0) and np.array_equal(attr_ref.decode(b1)[0], vals)
    assert Runtime.attr_info(b1) == attr_nl_ref.info(b1)
    b2 = attr2_ref.encode(pts, vals, bpv, p0=p0)
    ps, vs = K.morton(pts, vals)
    assert np.array_equal(K.head_of(b2)[4], p0) and np.array_equal(attr2_ref.decode(b2, pts)[0], vs)
    assert Runtime.attr_info(b2) == attr_nl_ref.info(b2)
    for k in range(16):
        assert Runtime.attr_lod_info(b2, k) == attr2_ref.lod_info(b2, k), k
    cells, want = K.sample(ps, vs, 2)
    assert np.array_equal(attr2_ref.decode(b2[:attr2_ref.lod_info(b2, 2)[0]], cells, 2)[0], want)
    for bad in (15, 4081):                                                # one step outside the table's range
        worse = bytearray(b2)
        struct.pack_into("<H", worse, attr2_ref.HEAD2 + 2 * 7, bad)
        with pytest.raises(pkg("_abi").PccError) as e:
            Runtime.attr_lod_info(bytes(worse), 0)
        assert e.value.code == pkg("_abi").PCC_E_STREAM and "initial probability %d" % bad in str(e.value)


def test_the_other_kinds_off_the_encoders_layout():
    """the kinds the GPU file decodes behind the lane decoder: near-lossless 4 and 7, cross-channel 8 and 11"""
    Runtime = pkg("runtime").Runtime
    pts, vals, bpv = K.frame("1000x3 uint8")
    ps, vs = K.morton(pts, vals)
    for lay in ((3, 6), (170, 1)):
        b4 = attr_nl_ref.encode(vals, bpv, 2, layout=lay)
        assert K.head_of(b4)[2:4] == lay and np.abs(attr_nl_ref.decode(b4, any_layout=True)[0] - vals).max() <= 2
        b8 = attr_cross_ref.encode(vals, bpv, True, layout=lay)
        assert K.head_of(b8)[2:4] == lay and np.array_equal(attr_cross_ref.decode(b8, any_layout=True)[0], vals)
        b13 = attr_cross_ref.encode(vals, bpv, True, e=3, layout=lay)
        assert K.head_of(b13)[2:4] == lay and np.abs(attr_cross_ref.decode(b13, any_layout=True)[0] - vals).max() <= 3
        b7 = attr_nl_ref.encode(vals, bpv, 2, points=pts, layout=lay)
        b11 = attr_cross_ref.encode(vals, bpv, True, points=pts, layout=lay)
        assert K.head_of(b7)[2:4] == lay and K.head_of(b11)[2:4] == lay
        assert np.abs(attr_nl_ref.decode(b7, pts, any_layout=True)[0] - vs).max() <= 2
        assert np.array_equal(attr_cross_ref.decode(b11, pts, any_layout=True)[0], vs)
        for b in (b4, b8, b13, b7, b11):
            assert Runtime.attr_info(b) == attr_cross_ref.info(b)
        for b in (b7, b11):
            for k in range(16):
                assert Runtime.attr_lod_info(b, k) == attr_cross_ref.lod_info(b, k, any_layout=True), k
            with pytest.raises(AssertionError):
                attr_cross_ref.lod_info(b, 1)
        with pytest.raises(AssertionError):
            attr_nl_ref.decode(b4)                                        # the default path: the encoder's layout


# (what, n, c, the layout the blob is written with, the (S, n_chunks) put into its header): each breaks one condition
OUTSIDE = [("S c = 513", 1000, 1, (512, 1), (513, 1)), ("S c = 514", 700, 2, (256, 1), (257, 1)),
           ("S c = 513, c = 3", 1000, 3, (170, 1), (171, 1)), ("S c = 516", 1000, 4, (128, 1), (129, 1)),
           ("S = 0", 1000, 3, (16, 1), (0, 1)),
           ("64 S nc = n - 1", 961, 3, (3, 6), (3, 5)), ("64 S (nc - 1) = n", 960, 3, (3, 5), (3, 6)),
           ("nc = n + 1", 1, 3, (1, 1), (1, 2)), ("nc = 0", 1000, 3, (16, 1), (16, 0))]


@pytest.mark.parametrize("what,n,c,good,bad", OUTSIDE, ids=[o[0] for o in OUTSIDE])
def test_one_step_outside_each_condition_is_refused(what, n, c, good, bad):
    """the header's S and n_chunks alone are changed: the parsers check them against n and c before they read the chunk
    table, so the refusal is the layout's (the message names n, n_chunks and S)"""
    abi, Runtime = pkg("_abi"), pkg("runtime").Runtime
    with pytest.raises(AssertionError):
        attr_ref.check_layout(n, c, *bad)
    pts, vals, bpv = K.frame((n, c, 1))
    blobs = {2: attr2_ref.encode(pts, vals, bpv, layout=good), 7: attr_nl_ref.encode(vals, bpv, 2, points=pts, layout=good)}
    if c > 1:
        blobs[11] = attr_cross_ref.encode(vals, bpv, True, points=pts, layout=good)
        blobs[14] = attr_cross_ref.encode(vals, bpv, True, e=2, points=pts, layout=good)
    for ver, blob in blobs.items():
        at = attr_ref.HEAD + 64 + (4 if ver in (7, 14) else 0)
        assert blob[1] == ver and struct.unpack_from("<II", blob, at) == good
        for lod in (0, 1):
            assert Runtime.attr_lod_info(blob, lod)[0] <= len(blob)
        worse = bytearray(blob)
        struct.pack_into("<II", worse, at, *bad)
        for lod in (0, 1):
            with pytest.raises(abi.PccError) as e:
                Runtime.attr_lod_info(bytes(worse), lod)
            assert e.value.code == abi.PCC_E_STREAM
            assert "%d points in %d chunks of 64 x %d" % (n, bad[1], bad[0]) in str(e.value), str(e.value)


def test_attr_info_refuses_a_layout_where_it_reads_one():
    """pcc_attr_info parses S and n_chunks only for the transform-coded kinds (versions 19, 21, 22; S behind qstep in 19)"""
    import attr_transform_ref
    abi, Runtime = pkg("_abi"), pkg("runtime").Runtime
    pts, vals, bpv = K.frame((960, 3, 1))
    blob = attr_transform_ref.encode(pts, vals, bpv, 4)
    at = attr_ref.HEAD + 4
    assert blob[1] == 19 and struct.unpack_from("<II", blob, at) == attr_ref.layout(960, 3) == (15, 1)
    assert Runtime.attr_info(blob)["points"] == 960
    for bad in ((171, 1), (14, 1), (15, 2), (15, 961), (0, 1)):
        worse = bytearray(blob)
        struct.pack_into("<II", worse, at, *bad)
        with pytest.raises(abi.PccError) as e:
            Runtime.attr_info(bytes(worse))
        assert e.value.code == abi.PCC_E_STREAM and "960 points in %d chunks of 64 x %d" % (bad[1], bad[0]) in str(e.value)
