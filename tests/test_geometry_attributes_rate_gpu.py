"""Transform-coded attributes under a byte target, on the GPU: compress(..., qstep=, target_bytes= /
target_frame_bytes=) against the existing call as the oracle.  For every frame and every rung of the ladder the oracle's
length is len(compress(..., qstep=ladder[j])[1][f]); the expected rung is tests/attr_rate_ref.py's search over those
lengths, and the budgeted call's blob must be the oracle's blob at that rung, byte for byte."""
import os

import numpy as np
import pytest

import attr_rate_ref as R
import attr_ref as A
from conftest import ROOT, pkg, random_cloud


@pytest.fixture(scope="module")
def geo():
    g = pkg().GeometryCodec()
    yield g
    g.close()


def _colour(rng, n, c, dtype):
    top = 1 << (8 * dtype.itemsize)
    step = 1 if dtype.itemsize == 1 else 97
    base = np.cumsum(rng.integers(-9, 10, n)) * step + rng.integers(0, top)
    return ((base[:, None] + rng.integers(-4, 5, (n, c)) * step) % top).astype(dtype)


def _cloud(rng, n):
    return random_cloud(rng, n, extent=48 if n < 5000 else 96, lo=-20)[:, 1:].astype(np.int32)


class _Oracle:
    """the existing call at every rung of the ladder: blobs[j][f], one call of all frames per rung"""

    def __init__(self, geo, frames, attrs, q, **kw):
        self.geo, self.frames, self.attrs, self.q, self.kw = geo, frames, attrs, q, kw
        c = attrs[0].shape[1]
        self.plain = isinstance(q, int) and "colour" not in kw                      # version 19
        self.ladder = pkg().GeometryCodec.rate_ladder(q, attrs[0].dtype, c)
        assert self.ladder == R.ladder(q, c, attrs[0].dtype.itemsize)
        self.J = len(self.ladder)
        self.geometry = None
        self.blobs = []
        for steps in self.ladder:
            gb, ab = geo.compress(frames, attributes=attrs, qstep=steps[0] if self.plain else steps, **kw)[:2]
            assert self.geometry in (None, gb)
            self.geometry = gb
            self.blobs.append(ab)

    def length(self, f, j):
        return len(self.blobs[j][f])

    def expect(self, f, target):
        """(rung, the rungs visited) of frame f; -1 for a frame without points"""
        if self.length(f, 0) == 12:
            return -1, []
        return R.choose(lambda j: self.length(f, j), self.J, target)

    def outcome(self, f, target):
        rung, seen = self.expect(f, target)
        if rung < 0:
            return "empty"
        if rung == 0:
            return "rung 0"
        if self.length(f, rung) > target:
            return "over"
        return "inside" if rung not in R.stage1(self.J) else ("a" if len(seen) > R.stage1(self.J).index(rung) + 1 else "a, no stage 2")

    def check(self, targets, frame_total=False, **more):
        """the budgeted call against the oracle; -> the rungs the frames got"""
        GeometryCodec = pkg().GeometryCodec
        key = "target_frame_bytes" if frame_total else "target_bytes"
        out = self.geo.compress(self.frames, attributes=self.attrs, qstep=self.q, **{key: targets}, **self.kw, **more)
        gb, ab = out[:2]
        assert gb == self.geometry
        rungs = []
        for f, t in enumerate(targets):
            if frame_total:
                t = max(1, t - len(gb[f]))
            rung, _ = self.expect(f, t)
            rungs.append(rung)
            want = self.blobs[max(rung, 0)][f]
            assert ab[f] == want, (f, t, rung, len(ab[f]), len(want), [self.length(f, j) for j in range(self.J)])
            info = GeometryCodec.attr_info(ab[f])
            if rung < 0:
                assert len(ab[f]) == 12
            elif self.plain:
                assert info["version"] == 19 and info["qstep"] == self.ladder[rung][0]
            else:
                assert info["version"] == 21 and info["qstep"] == self.ladder[rung]
                assert info["colour"] == self.kw.get("colour")
            if rung >= 0 and any(self.length(f, j) <= t for j in R.stage1(self.J)):
                assert len(ab[f]) <= t                       # the bound holds wherever a rung of A fits
        return rungs, out


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        return [f[f"points_{i}"].astype(np.int32) for i in range(4)], [f[f"colors_u8_{i}"] for i in range(4)]


@pytest.fixture(scope="module")
def recorded_colour(geo, recorded):
    return _Oracle(geo, recorded[0], recorded[1], (4, 8, 8), colour="ycocg")


@pytest.mark.gpu
def test_recorded_frames_meet_all_four_outcomes(geo, recorded_colour):
    """frames 0 .. 3 (19-20k points: two chunks each) in one call, qstep (4, 8, 8) with the colour transform"""
    o = recorded_colour
    J = o.J
    assert J == 21 and all(len(o.frames[f]) > 10880 for f in range(4))
    assert [o.length(0, j) for j in range(J)] == [15216, 14828, 13084, 12120, 10548, 9776, 8722, 7922, 7064, 6360, 5628, 5066, 4534, 4060,
                                                  3604, 3260, 2934, 2654, 2430, 2276, 2144]
    targets = [o.length(0, 0), o.length(1, J - 1) - 1, o.length(2, 6), o.length(3, 8)]
    outcomes = [o.outcome(f, t) for f, t in enumerate(targets)]
    assert outcomes == ["rung 0", "over", "inside", "a"], outcomes
    rungs, (gb, ab) = o.check(targets)
    assert rungs[0] == 0 and rungs[1] == J - 1 and len(ab[1]) == targets[1] + 1 and rungs[3] == 8
    assert rungs[2] == o.expect(2, targets[2])[0] and 4 < rungs[2] < 8
    pts, vals = geo.decompress(gb, ab)
    wpts, wvals = geo.decompress(gb, [o.blobs[r][f] for f, r in enumerate(rungs)])
    assert all(np.array_equal(a, b) for a, b in zip(pts, wpts)) and all(np.array_equal(a, b) for a, b in zip(vals, wvals))
    # frame 0 at 6000 bytes: rung 10, steps (23, 46, 46)
    assert o.check([6000, 6000, 6000, 6000])[0][0] == 10


@pytest.mark.gpu
def test_recorded_frames_under_one_integer_step(geo, recorded):
    """qstep = 8 without colour: version 19, the same identity"""
    o = _Oracle(geo, recorded[0], recorded[1], 8)
    assert o.J == 17
    rungs, _ = o.check([o.length(0, 5), o.length(1, 0) + 100, 1, o.length(3, 12) + 1])
    assert rungs[1] == 0 and rungs[2] == 16
    o.check([7000] * 4)


@pytest.mark.gpu
def test_a_budget_for_geometry_and_attributes_together(geo, recorded_colour):
    o = recorded_colour
    g = [len(b) for b in o.geometry]
    totals = [g[0] + o.length(0, 3), g[1] - 5, g[2] + 6000, g[3] + o.length(3, 20)]
    rungs, (gb, ab) = o.check(totals, frame_total=True)
    assert rungs[1] == o.J - 1 and rungs[3] == 20
    for f in (0, 2, 3):
        assert len(gb[f]) + len(ab[f]) <= totals[f]
    assert ab == geo.compress(o.frames, attributes=o.attrs, qstep=o.q, colour="ycocg",
                              target_bytes=[max(1, t - n) for t, n in zip(totals, g)])[1]


@pytest.mark.gpu
def test_the_scratch_limit_changes_no_byte(geo, recorded_colour):
    """one row per group (and the winners coded once more), two rows per group, and the default"""
    o = recorded_colour
    targets = [6000, o.length(1, 0), 3000, 100]
    want = o.check(targets)[1][1]
    try:
        for limit in (1, 10_000_000):
            geo.rate_scratch_limit = limit
            assert o.check(targets)[1][1] == want, limit
    finally:
        geo.rate_scratch_limit = 0


@pytest.mark.gpu
def test_small_frames_in_one_call(geo):
    """1, 2, 64 points, no points, 65 points: n = 1 has one length at every rung, so rung 0 or J - 1"""
    rng = np.random.default_rng(77)
    dtype = np.dtype(np.uint8)
    frames = [_cloud(rng, 1), _cloud(rng, 2), _cloud(rng, 64), np.zeros((0, 3), np.int32), _cloud(rng, 65)]
    attrs = [_colour(rng, len(p), 3, dtype) for p in frames]
    o = _Oracle(geo, frames, attrs, (4, 8, 8), colour="ycocg")
    assert len({o.length(0, j) for j in range(o.J)}) == 1
    one = o.length(0, 0)
    rungs, _ = o.check([one, o.length(1, 9), o.length(2, 6), 1, o.length(4, 19)])
    assert rungs[0] == 0 and rungs[3] == -1
    rungs, _ = o.check([one - 1, 10 ** 6, o.length(2, 13), 50, o.length(4, 2)])
    assert rungs[0] == o.J - 1 and rungs[1] == 0 and rungs[3] == -1


def _check_with_rungs(o, targets, monkeypatch):
    """o.check(targets), and the rungs the library itself reported for the call"""
    got = []
    real = o.geo.rt.attr_encode_frames_rate

    def record(*a, **k):
        blobs, rungs = real(*a, **k)
        got.append(list(rungs))
        return blobs, rungs

    with monkeypatch.context() as m:
        m.setattr(o.geo.rt, "attr_encode_frames_rate", record)
        want, (gb, ab) = o.check(targets)
    assert got == [want], (got, want)
    return want, ab


def _row_need(n, c, bpv):
    """scratch bytes of one candidate row: its indices and its two regions of one word per decision, each on 256 bytes"""
    S, nc = A.layout(n, c)
    words = nc * A.LANES * S * c * A.positions(bpv)
    return -(-n * c * 2 // 256) * 256 + 2 * (-(-words * 2 // 256) * 256)


@pytest.mark.gpu
def test_small_frames_under_a_scratch_limit(geo, monkeypatch):
    """test_small_frames_in_one_call's frames with the candidate rows in groups: an empty frame between frames whose
    winners are coded once more"""
    rng = np.random.default_rng(77)
    dtype = np.dtype(np.uint8)
    frames = [_cloud(rng, 1), _cloud(rng, 2), _cloud(rng, 64), np.zeros((0, 3), np.int32), _cloud(rng, 65)]
    attrs = [_colour(rng, len(p), 3, dtype) for p in frames]
    o = _Oracle(geo, frames, attrs, (4, 8, 8), colour="ycocg")
    one = o.length(0, 0)
    lists = [[one, o.length(1, 9), o.length(2, 6), 1, o.length(4, 19)], [one - 1, 10 ** 6, o.length(2, 13), 50, o.length(4, 2)]]
    # a row's scratch from its frame's distinct points; twice the largest row's: every group holds two rows or more,
    # and stage 1 alone (its rungs for each of the four frames with points) needs several times as much
    need = [_row_need(len(np.unique(p, axis=0)), 3, 1) for p in frames if len(p)]
    middle = 2 * max(need)
    assert middle < len(R.stage1(o.J)) * sum(need) // 2
    want = [_check_with_rungs(o, targets, monkeypatch) for targets in lists]
    assert [w[0][3] for w in want] == [-1, -1] and want[0][0][0] == 0 and want[1][0][0] == o.J - 1
    try:
        for limit in (1, middle):
            geo.rate_scratch_limit = limit
            for targets, (rungs, blobs) in zip(lists, want):
                assert _check_with_rungs(o, targets, monkeypatch) == (rungs, blobs), limit
    finally:
        geo.rate_scratch_limit = 0


@pytest.mark.gpu
def test_two_chunks_under_a_scratch_limit_between_empty_frames(geo, monkeypatch):
    """test_four_channels_across_the_chunk_boundary's frame with a frame without points in front of it and behind it"""
    rng = np.random.default_rng(78)
    empty = np.zeros((0, 3), np.int32)
    frames = [empty, _cloud(rng, 8193), empty]
    attrs = [np.zeros((0, 4), np.uint8), _colour(rng, 8193, 4, np.dtype(np.uint8)), np.zeros((0, 4), np.uint8)]
    o = _Oracle(geo, frames, attrs, (4, 8, 8, 16), colour="ycocg")
    assert o.J == 21
    try:
        for limit in (1, 0):
            geo.rate_scratch_limit = limit
            for k in (7, 20):
                rungs, ab = _check_with_rungs(o, [1, o.length(1, k), 10 ** 6], monkeypatch)
                assert rungs == [-1, k, -1] and len(ab[0]) == len(ab[2]) == 12, (limit, k, rungs)
    finally:
        geo.rate_scratch_limit = 0


@pytest.mark.gpu
def test_four_channels_across_the_chunk_boundary(geo):
    """c = 4 at 8193 points, the first frame of two chunks"""
    rng = np.random.default_rng(78)
    frames = [_cloud(rng, 8193)]
    attrs = [_colour(rng, 8193, 4, np.dtype(np.uint8))]
    o = _Oracle(geo, frames, attrs, (4, 8, 8, 16), colour="ycocg")
    assert o.J == 21
    for k in (7, 12, 20):
        o.check([o.length(0, k)])


@pytest.mark.gpu
def test_uint16_one_channel(geo):
    """uint16, c = 1, qstep 1: 61 rungs"""
    rng = np.random.default_rng(79)
    frames = [_cloud(rng, 300), _cloud(rng, 65)]
    attrs = [_colour(rng, len(p), 1, np.dtype(np.uint16)) for p in frames]
    o = _Oracle(geo, frames, attrs, 1)
    assert o.J == 61
    o.check([o.length(0, 30), o.length(1, 59)])
    o.check([o.length(0, 57) - 1, o.length(1, 0)])
    o.check([1, o.length(1, 41)])


@pytest.mark.gpu
def test_the_senders_side_of_a_level_of_detail(geo):
    rng = np.random.default_rng(80)
    frames = [_cloud(rng, 3000), _cloud(rng, 300)]
    attrs = [_colour(rng, len(p), 3, np.dtype(np.uint8)) for p in frames]
    o = _Oracle(geo, frames, attrs, 6, colour="ycocg", lod=2)
    rungs, (gb, ab) = o.check([o.length(0, 6), o.length(1, 11)])
    assert all(pkg().GeometryCodec.attr_info(b)["lod"] == 2 for b in ab)


@pytest.mark.gpu
def test_float32_frames_that_lose_rows(geo):
    rng = np.random.default_rng(81)
    voxel, origin = 0.05, (1.0, -2.0, 0.5)
    lats = [_cloud(rng, 3000), _cloud(rng, 700), _cloud(rng, 5)]
    attrs = [_colour(rng, len(p), 3, np.dtype(np.uint8)) for p in lats]
    fl = [(p.astype(np.float32) * np.float32(voxel) + np.asarray(origin, np.float32)).astype(np.float32) for p in lats]
    for f in fl[:2]:
        rows = rng.permutation(f.shape[0])[:f.shape[0] // 10]
        f[rows, rng.integers(0, 3, rows.size)] = np.nan
    fl[2][:] = np.nan                                                       # a frame that loses every row
    o = _Oracle(geo, fl, attrs, 5, voxel=voxel, origin=origin, invalid="drop")
    rungs, out = o.check([o.length(0, 7), o.length(1, 2), 40], return_index=True)
    assert rungs[2] == -1 and len(out) == 3
    plain = geo.compress(fl, attributes=attrs, qstep=5, voxel=voxel, origin=origin, invalid="drop", return_index=True)
    assert all(np.array_equal(a, b) for a, b in zip(out[2], plain[2]))


@pytest.mark.gpu
def test_errors_leave_the_codec_usable(geo, recorded_colour, monkeypatch):
    abi = pkg("_abi")
    o = recorded_colour
    real = geo.rt.attr_encode_frames_rate
    with monkeypatch.context() as m:
        m.setattr(geo.rt, "attr_encode_frames_rate", lambda *a, **k: real(*a, cap=5000, **k))
        with pytest.raises(abi.PccError, match="capacity 5000") as e:
            o.check([6000] * 4)
        assert e.value.code == abi.PCC_E_NOMEM
    o.check([6000] * 4)
    with monkeypatch.context() as m:
        m.setattr(geo.rt, "attr_encode_frames_rate", lambda *a, **k: real(*a[:13], [6000, 6000, 0, 6000], *a[14:], **k))
        with pytest.raises(abi.PccError, match="frame 2: a target of 0 bytes") as e:
            o.check([6000] * 4)
        assert e.value.code == abi.PCC_E_ARG
    o.check([6000] * 4)
