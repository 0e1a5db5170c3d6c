"""GeometryCodec.filter and the outlier kernels on the device (csrc/outlier.h behind csrc/knn.hip), held integer for
integer and byte for byte to tests/outlier_ref.py on the cases of tests/test_geometry_filter.py — among them the calls of
70 + 58 + 1 points whose frame boundaries fall inside a wave — then filter end to end, its composition with compress, and
the refusals.  Every shape is at most 20 000 points."""
import ctypes as C
import os

import numpy as np
import pytest

import nn_ref
import outlier_ref
from conftest import ROOT, pkg
from test_geometry_filter import CASES, KS, MS, RADII, _random, _surface, case, planted


def _dev(rt, keys):
    import torch
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(rt.device)


@pytest.fixture(scope="module")
def geo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg().GeometryCodec()
    yield g
    g.close()


# ------------------------------------------------------------------ the kernels against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CASES)
def test_scores_sums_and_masks_on_the_device(rt, name, k):
    c = case(name)
    nf = len(c.frames)
    want_q, want_sums = c.scores(k)
    keys = _dev(rt, c.keys)
    scores, sums = rt.outlier_scores_frames(keys, nf, k)
    assert np.array_equal(scores.cpu().numpy().view(np.uint64), want_q)
    assert sums == want_sums
    for std_ratio in (0.5, 2.0):
        r = rt.outlier_ratio(std_ratio)
        th = [rt.outlier_threshold(n, s1, s2, r) for s1, s2, n in sums]
        assert th == [outlier_ref.threshold(want_q[c.frame_of == f].tolist(), r) for f in range(nf)]
        keep, kept = rt.outlier_mask_frames(keys, nf, scores, th)
        rt.sync()
        want_keep = want_q <= np.array(th, dtype=np.uint64)[c.frame_of]
        assert np.array_equal(keep.cpu().numpy(), want_keep.astype(np.uint8))
        assert kept.cpu().tolist() == [int(want_keep[c.frame_of == f].sum()) for f in range(nf)]


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", CASES)
def test_radius_rule_on_the_device(rt, name, m):
    c = case(name)
    nf = len(c.frames)
    keys = _dev(rt, c.keys)
    for radius2 in RADII + (1 << 70,):
        keep, counts = rt.outlier_radius_frames(keys, nf, m, radius2)
        rt.sync()
        want = c.radius(m, radius2)
        assert np.array_equal(keep.cpu().numpy(), want), radius2
        assert counts.cpu().tolist() == [[int((c.frame_of == f).sum()), int(want[c.frame_of == f].sum())] for f in range(nf)]


@pytest.mark.gpu
def test_planted_outliers_on_the_device(geo):
    rows, is_plant = planted()
    (kept,), (mask,), (rep,) = geo.filter([rows.astype(np.int32)], k=16, std_ratio=2, return_mask=True, return_report=True)
    want, distinct, keep = outlier_ref.filter_rows(rows, lambda p: outlier_ref.statistical(p, 16, 2.0)[0])
    assert np.array_equal(mask, want) and np.array_equal(kept, rows[want])
    assert not mask[is_plant].any() and mask[~is_plant].mean() >= 0.97
    assert rep["points"] == distinct.shape[0] and rep["kept"] == int(keep.sum()) and rep["rows_kept"] == int(want.sum())


# ------------------------------------------------------------------ filter end to end
def _call_frames():
    """the rows of one call: a surface with three far points, every fifth row given twice, shuffled; an empty frame; a
    frame of one point and one of two; a random cloud; an empty frame at the end"""
    rng = np.random.default_rng(11)
    a = np.concatenate([_surface(12, 400), [[300, -200, 150], [-250, 280, 90], [310, 310, -310]]])
    a = np.concatenate([a, a[::5]])
    a = a[rng.permutation(a.shape[0])]
    return [a, np.zeros((0, 3), np.int64), np.array([[5, -6, 7]]), np.array([[1, 2, 3], [2, 2, 3]]), _random(13, 65) * 2,
            np.zeros((0, 3), np.int64)]


METHODS = {"statistical": (dict(method="statistical", k=8, std_ratio=1.5), lambda p: outlier_ref.statistical(p, 8, 1.5)[0]),
           "radius": (dict(method="radius", min_neighbours=2, radius2=9), lambda p: outlier_ref.radius(p, 2, 9))}


@pytest.fixture(scope="module")
def call():
    frames = _call_frames()
    return frames, {name: [outlier_ref.filter_rows(f, fn) for f in frames] for name, (_, fn) in METHODS.items()}


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


@pytest.mark.gpu
@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("dtype", ["int16", "int32", "float32"])
@pytest.mark.parametrize("place", ["host", "device"])
def test_filter_follows_the_input_rows(geo, call, place, dtype, method):
    import torch
    frames, want = call
    kw, _ = METHODS[method]
    kw = dict(kw)
    if dtype == "float32":      # x = origin + q * voxel, exact in float32: the lattice is the same
        given = [(f * 0.25 + np.array([1.0, -2.0, 0.5])).astype(np.float32) for f in frames]
        kw.update(voxel=0.25, origin=(1.0, -2.0, 0.5))
    else:
        given = [f.astype(dtype) for f in frames]
    inputs = [torch.from_numpy(g).to(geo.rt.device) for g in given] if place == "device" else given
    results = {}
    for output in ("numpy", "device"):
        kept, mask, report = geo.filter(inputs, return_mask=True, return_report=True, output=output, **kw)
        if output == "device":
            assert all(isinstance(t, torch.Tensor) and t.device == geo.rt.device for t in kept + mask)
        results[output] = ([_np(a) for a in kept], [_np(a) for a in mask])
        for f, (g, (w_mask, distinct, keep)) in enumerate(zip(given, want[method])):
            got, m = results[output][0][f], results[output][1][f]
            assert m.dtype == np.bool_ and np.array_equal(m, w_mask), f
            assert got.dtype == g.dtype and np.array_equal(got, g[w_mask]), f      # the caller's rows, in input order
            rep = report[f]
            assert (rep["points"], rep["kept"], rep["rows_kept"]) == (distinct.shape[0], int(keep.sum()), int(w_mask.sum())), f
            assert all(type(v) is int for v in rep.values())
            if method == "statistical":
                ref = outlier_ref.statistical(distinct, 8, 1.5)[1]
                assert {k: rep[k] for k in ("k_eff", "S1", "S2", "threshold")} == {k: ref[k] for k in ("k_eff", "S1", "S2", "threshold")}
    # duplicates share a verdict; the edge frames
    masks = results["numpy"][1]
    rows = [tuple(r) for r in frames[0].tolist()]
    verdict = {}
    for r, v in zip(rows, masks[0].tolist()):
        assert verdict.setdefault(r, v) == v
    assert masks[1].shape == (0,) and results["numpy"][0][1].shape == (0, 3) and masks[5].shape == (0,)
    assert masks[2].tolist() == [method == "statistical"]      # one point: kept whole / dropped whole
    assert masks[3].tolist() == ([True, True] if method == "statistical" else [False, False])


@pytest.mark.gpu
def test_filter_drops_invalid_rows(geo):
    pts = (_surface(21, 200) * 0.5).astype(np.float32)
    pts[[3, 77]] = np.nan
    kept, mask = geo.filter([pts], voxel=0.5, invalid="drop", return_mask=True, k=8)
    ok = np.isfinite(pts).all(1)
    want, _, _ = outlier_ref.filter_rows(np.rint(pts[ok] / 0.5).astype(np.int64), lambda p: outlier_ref.statistical(p, 8, 2.0)[0])
    assert not mask[0][~ok].any() and np.array_equal(mask[0][ok], want)
    assert np.array_equal(kept[0], pts[mask[0]])
    with pytest.raises(pkg("_abi").PccError, match="non-finite"):
        geo.filter([pts], voxel=0.5)
    none = geo.filter([pts[[3, 77]]], voxel=0.5, invalid="drop", return_mask=True, return_report=True, method="radius", radius2=4)
    assert none[0][0].shape == (0, 3) and none[1][0].tolist() == [False, False] and none[2] == [{"points": 0, "kept": 0, "rows_kept": 0}]


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["host", "device"])
def test_filter_returns_the_attribute_rows_as_given(geo, call, place):
    import torch
    frames, want = call
    rng = np.random.default_rng(3)
    masks = [w[0] for w in want["radius"]]
    given = [f.astype(np.int32) for f in frames]
    dev = lambda a: torch.from_numpy(a).to(geo.rt.device) if place == "device" else a
    sets = {"uint8 rgb": [rng.integers(0, 256, (f.shape[0], 3), dtype=np.uint8) for f in frames],
            "uint16 flat": [rng.integers(0, 65536, f.shape[0], dtype=np.uint16) for f in frames],
            "uint16 four": [rng.integers(0, 65536, (f.shape[0], 4), dtype=np.uint16) for f in frames],
            "float32 two": [rng.random((f.shape[0], 2), dtype=np.float32) for f in frames],
            "float64 rgb": [rng.random((f.shape[0], 3)) for f in frames]}
    wide = [rng.integers(0, 256, (f.shape[0], 8), dtype=np.uint8) for f in frames]
    for name, attrs in list(sets.items()) + [("pitched view", None)]:
        if attrs is None:      # [:, 4:7] of rows of 8 bytes: goes in by its pitch
            attrs, passed = [w[:, 4:7] for w in wide], [dev(w)[:, 4:7] for w in wide]
        else:
            passed = [dev(a) for a in attrs]
        for output in ("numpy", "device"):
            kept, out = geo.filter([dev(g) for g in given], attributes=passed, method="radius", min_neighbours=2, radius2=9, output=output)
            for f, (a, m) in enumerate(zip(attrs, masks)):
                got = _np(out[f])
                assert got.dtype == a.dtype and got.shape == a[m].shape and np.array_equal(got, a[m]), (name, output, f)
                assert np.array_equal(_np(kept[f]), given[f][m])
    # host frames with device attributes, and the other way round
    kept, out = geo.filter(given, attributes=[torch.from_numpy(a).to(geo.rt.device) for a in sets["uint8 rgb"]], method="radius",
                           min_neighbours=2, radius2=9)
    assert all(np.array_equal(o, a[m]) for o, a, m in zip(out, sets["uint8 rgb"], masks))


@pytest.mark.gpu
def test_filter_then_compress_round_trips(geo, call):
    frames, want = call
    given = [f.astype(np.int32) for f in frames]
    kept = geo.filter(given, k=8, std_ratio=1.5)
    back = geo.decompress(geo.compress(kept))
    on_device = geo.decompress(geo.compress(geo.filter([__import__("torch").from_numpy(g).to(geo.rt.device) for g in given], k=8,
                                                       std_ratio=1.5, output="device")))
    for f, (k, b, d) in enumerate(zip(kept, back, on_device)):
        uniq = np.unique(k, axis=0)
        assert np.array_equal(np.unique(b, axis=0), uniq) and b.shape == uniq.shape, f
        assert np.array_equal(d, b)


@pytest.mark.gpu
def test_filtered_camera_frame_codes_shorter(geo):
    """recorded camera frame 0 (19 679 points): fewer bytes, and not more bytes per point kept"""
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as z:
        pts = z["points_0"]
    kept, report = geo.filter([pts], return_report=True)
    (whole,), (filtered,) = geo.compress([pts]), geo.compress(kept)
    n, n_kept = report[0]["points"], report[0]["kept"]
    print(f"zed frame 0: {n} points {len(whole)} B -> {n_kept} points {len(filtered)} B")
    assert 0 < n_kept < n
    assert len(filtered) < len(whole)
    assert len(filtered) * n <= len(whole) * n_kept      # bytes per point kept


# ------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_outlier_refusals_launch_nothing(rt):
    import torch
    abi = pkg("_abi")
    pts = nn_ref.morton_sorted_unique(np.random.default_rng(4).integers(-50, 50, (200, 3)))
    good = nn_ref.morton_keys(pts)
    n = good.shape[0]
    d_good = _dev(rt, good)
    bad = {"not sorted": (good[::-1], 1, 8, abi.PCC_E_ARG), "duplicate": (np.repeat(good, 2)[:n], 1, 8, abi.PCC_E_DUP),
           "frame index": (nn_ref.morton_keys(pts, 2), 2, 8, abi.PCC_E_RANGE), "k=2": (good, 1, 2, abi.PCC_E_ARG),
           "k=33": (good, 1, 33, abi.PCC_E_ARG), "n_frames=0": (good, 0, 8, abi.PCC_E_ARG),
           "n_frames=65536": (good, 65536, 8, abi.PCC_E_ARG)}
    want_q = np.array(outlier_ref.scores(pts, 8), dtype=np.uint64)
    for word, (keys, n_frames, k, code) in bad.items():
        scores = torch.full((n,), 7, dtype=torch.int64, device=rt.device)
        sums = torch.full((max(1, min(n_frames, 4)), 4), 7, dtype=torch.int64, device=rt.device)
        keep = torch.full((n,), 7, dtype=torch.uint8, device=rt.device)
        d = _dev(rt, keys)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        rc = rt.lib.pcc_outlier_scores_frames(rt.ctx, ptr(d), n, n_frames, k, ptr(scores), ptr(sums))
        assert rc == code and word.encode() in rt.lib.pcc_last_error(), (word, rc, rt.lib.pcc_last_error())
        m = {2: 0, 33: 32}.get(k, k)      # the radius entry's range is 1 .. 31
        rc = rt.lib.pcc_outlier_radius_frames(rt.ctx, ptr(d), n, n_frames, m, 9, ptr(keep), ptr(sums))
        assert rc == code, (word, rc, rt.lib.pcc_last_error())
        assert (word if "k=" not in word else "min_neighbours in 1 .. 31").encode() in rt.lib.pcc_last_error()
        if "k=" not in word:
            rc = rt.lib.pcc_outlier_mask_frames(rt.ctx, ptr(d), n, n_frames, ptr(scores), ptr(sums), ptr(keep), ptr(sums))
            assert rc == code and word.encode() in rt.lib.pcc_last_error(), (word, rc, rt.lib.pcc_last_error())
        rt.sync()
        assert bool((scores == 7).all()) and bool((sums == 7).all()) and bool((keep == 7).all()), word
        with pytest.raises(abi.PccError, match=word if "k=" not in word else "k in 3 .. 32"):
            rt.outlier_scores_frames(d, n_frames, k)
        got, _ = rt.outlier_scores_frames(d_good, 1, 8)      # a clean call follows
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want_q)
    rc = rt.lib.pcc_outlier_scores_frames(rt.ctx, None, (1 << 27) + 1, 1, 8, None, None)
    assert rc == abi.PCC_E_ARG and b"2^27" in rt.lib.pcc_last_error()
    scores, sums = rt.outlier_scores_frames(d_good[:0], 3, 8)      # n = 0 launches nothing and zeroes the sums
    assert scores.shape == (0,) and sums == [(0, 0, 0)] * 3


@pytest.mark.gpu
def test_filter_refusals_leave_the_codec_usable(geo):
    abi = pkg("_abi")
    pts = _surface(31, 100).astype(np.int32)
    want = geo.filter([pts], k=8)
    for call in (lambda: geo.filter([pts], k=2), lambda: geo.filter([pts], method="radius"),
                 lambda: geo.filter([pts], attributes=[np.zeros((5, 3), np.uint8)])):
        with pytest.raises(ValueError):
            call()
        assert np.array_equal(geo.filter([pts], k=8)[0], want[0])
    with pytest.raises(abi.PccError, match="outside"):
        geo.filter([np.array([[0, 0, 40000]], np.int32)])
    assert np.array_equal(geo.filter([pts], k=8)[0], want[0])
