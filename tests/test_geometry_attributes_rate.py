"""Transform-coded attributes under a byte target (compress(..., qstep=, target_bytes= / target_frame_bytes=);
include/pcc.h has the ladder and the search), on the host: the ladder's known answers from the numpy restatement
tests/attr_rate_ref.py and from the library, the search against hand-made length tables, the restatement on a recorded
camera frame, and what compress refuses before it enters the runtime.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import attr_rate_ref as R
import attr_ref
from conftest import ROOT, pkg
from test_geometry_attributes_lod import _morton

GeometryCodec = pkg().GeometryCodec

U8_32 = [32, 38, 46, 54, 64, 76, 92, 108, 127]
U8_1 = [1, 1, 1, 1, 2, 2, 2, 3, 4, 4, 5, 6, 8, 9, 11, 13, 16, 19, 23, 27, 32, 38, 46, 54, 64, 76, 92, 108, 127]


@pytest.mark.parametrize("ladder", [R.ladder, lambda q, c, bpv: GeometryCodec.rate_ladder(q, np.uint8 if bpv == 1 else np.uint16, c)],
                         ids=["restatement", "library"])
def test_ladder_known_answers(ladder):
    assert [s[0] for s in ladder(32, 1, 1)] == U8_32
    assert [s[0] for s in ladder(1, 1, 1)] == U8_1
    rgb = ladder((4, 8, 8), 3, 1)
    assert len(rgb) == 21 and rgb[0] == (4, 8, 8) and rgb[10] == (23, 46, 46) and rgb[16] == (64, 127, 127) and rgb[20] == (127, 127, 127)
    assert all(len(set(r)) > 1 for r in rgb[:20])          # the first rung with every step at H - 1 is the last
    wide = ladder(1, 1, 2)
    assert len(wide) == 61 and wide[0] == (1,) and wide[-1] == (32767,) and wide[-2] != (32767,)
    assert ladder(7, 4, 1)[0] == (7, 7, 7, 7)              # an integer serves every channel


def test_ladder_refusals():
    abi = pkg("_abi")
    for q, c, bpv in ((128, 1, 1), (0, 1, 1), (32768, 1, 2), ((4, 4, 200), 3, 1)):
        with pytest.raises(AssertionError):
            R.ladder(q, c, bpv)
        with pytest.raises(abi.PccError, match="qstep") as e:
            GeometryCodec.rate_ladder(q, np.uint8 if bpv == 1 else np.uint16, c)
        assert e.value.code == abi.PCC_E_ARG
    steps, out, J = (C.c_int32 * 4)(4, 4, 4, 4), (C.c_int32 * 256)(), C.c_int32(0)
    for c in (0, 5, -1):
        with pytest.raises(AssertionError):
            R.ladder(4, c, 1)
        assert abi.lib().pcc_attr_rate_ladder(steps, c, 1, out, C.byref(J)) == abi.PCC_E_ARG
    assert abi.lib().pcc_attr_rate_ladder(steps, 3, 3, out, C.byref(J)) == abi.PCC_E_ARG
    assert abi.lib().pcc_attr_rate_ladder(steps, 3, 1, out, C.byref(J)) == abi.PCC_OK and J.value == 21
    with pytest.raises(ValueError, match="3 steps for 4 channels"):
        GeometryCodec.rate_ladder((4, 8, 8), np.uint8, 4)
    with pytest.raises(TypeError, match="uint8 or uint16"):
        GeometryCodec.rate_ladder(4, np.int16)


def test_abi_is_declared_and_bound():
    abi = pkg("_abi")
    with open(os.path.join(ROOT, "include", "pcc.h")) as f:
        text = f.read()
    for name in ("pcc_attr_rate_ladder", "pcc_attr_encode_frames_rate"):
        assert name in abi.PROTOTYPES and name + "(" in text, name
        assert getattr(abi.lib(), name) is not None


def _choose(table, target):
    return R.choose(lambda j: table[j], len(table), target)


def test_the_search_on_hand_made_tables():
    J = 11                                                  # A = 0 4 8 10
    assert R.stage1(J) == [0, 4, 8, 10] and R.stage1(9) == [0, 4, 8] and R.stage1(1) == [0] and R.stage1(2) == [0, 1]
    down = [100 - 5 * j for j in range(J)]                  # 100 95 .. 50
    assert _choose(down, 100) == (0, [0])                                       # rung 0
    assert _choose(down, 1000) == (0, [0])
    assert _choose(down, 72) == (6, [0, 4, 8, 5, 6])                            # an interior rung from stage 2
    assert _choose(down, 60) == (8, [0, 4, 8, 5, 6, 7])                         # stage 2 finds none: a
    assert _choose(down, 55) == (9, [0, 4, 8, 10, 9])                           # the short last interval
    assert _choose(down, 50) == (10, [0, 4, 8, 10, 9])
    assert _choose(down, 49) == (10, [0, 4, 8, 10])                             # nothing fits: J - 1, over its target
    assert _choose([30], 5) == (0, [0]) and _choose([30, 30], 5) == (1, [0, 1])
    # not monotone: the procedure is the rule, not "the finest rung that fits".  Rungs 2 and 5 both fit 75; stage 1
    # passes rung 4 (80) and stops at rung 8, so stage 2 looks inside (4, 8) only and the frame gets rung 5
    bumpy = [100, 90, 70, 95, 80, 60, 61, 59, 40, 41, 39]
    assert _choose(bumpy, 75) == (5, [0, 4, 8, 5])
    assert min(j for j in range(J) if bumpy[j] <= 75) == 2
    assert _choose(bumpy, 40) == (8, [0, 4, 8, 5, 6, 7])                        # 10 fits too and is shorter; the search stops at 8
    assert _choose(bumpy, 92) == (1, [0, 4, 1])


def _zed(i):
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        u, mean = attr_ref.merge(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"])
    return _morton(u, mean)


ZED0 = [15216, 14828, 13084, 12120, 10548, 9776, 8722, 7922, 7064, 6360, 5628, 5066, 4534, 4060, 3604, 3260, 2934, 2654, 2430, 2276, 2144]


def test_the_restatement_on_a_recorded_frame():
    """frame 0 (19 679 points), qstep (4, 8, 8) with the colour transform, 6000 bytes: stage 1 walks rungs 0 4 8 12
    (15216 10548 7064 4534), stage 2 rungs 9 and 10 (6360, 5628), and the frame gets rung 10, steps (23, 46, 46)"""
    pts, vals = _zed(0)
    vals = np.asarray(vals, np.int64)
    assert len(pts) == 19679
    blob, rung, seen = R.encode(pts, vals, 1, (4, 8, 8), 6000, 1)
    assert (rung, seen) == (10, [0, 4, 8, 12, 9, 10]) and len(blob) == ZED0[10] == 5628
    info = GeometryCodec.attr_info(blob)
    assert info["version"] == 21 and info["qstep"] == (23, 46, 46) == R.ladder((4, 8, 8), 3, 1)[10] and info["colour"] == "ycocg"
    assert blob == R.encode_at(pts, vals, 1, (23, 46, 46), 1)
    assert R.choose(lambda j: ZED0[j], 21, 6000)[0] == 10 and all(a > b for a, b in zip(ZED0, ZED0[1:]))


def test_compress_checks_the_targets():
    """the checks of compress that run before the runtime is entered: on an instance that has none"""
    geo = object.__new__(GeometryCodec)
    pts = [np.zeros((3, 3), np.int32) + np.arange(3, dtype=np.int32)[:, None]] * 2
    a8 = np.zeros((3, 3), np.uint8)
    for name in ("target_bytes", "target_frame_bytes"):
        for bad in (True, 100.0, "100", [100, 2.5], (100, False), np.float32(9)):
            with pytest.raises(TypeError, match=name):
                geo.compress(pts, attributes=[a8, a8], qstep=4, **{name: bad})
        with pytest.raises(ValueError, match="frame 0: " + name + " must be at least 1, got 0"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, **{name: 0})
        with pytest.raises(ValueError, match="frame 1: " + name + " must be at least 1, got -3"):
            geo.compress(pts, attributes=[a8, a8], qstep=(4, 8, 8), colour="ycocg", **{name: [5, -3]})
        with pytest.raises(ValueError, match=name + " has 3 entries for 2 frames"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, **{name: [100, 100, 100]})
        with pytest.raises(ValueError, match="needs qstep"):
            geo.compress(pts, attributes=[a8, a8], **{name: 100})
        with pytest.raises(ValueError, match="needs qstep"):
            geo.compress(pts, **{name: 100})
        with pytest.raises(ValueError, match="needs qstep"):
            geo.compress(pts, attributes=[a8, a8], max_error=2, **{name: 100})
        with pytest.raises(ValueError, match=name + " with scalable_to"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, scalable_to=2, **{name: 100})
        with pytest.raises(ValueError, match="qstep with max_error"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, max_error=2, **{name: 100})
        with pytest.raises(ValueError, match="qstep with scalable=True"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, scalable=True, **{name: 100})
        with pytest.raises(ValueError, match="qstep with cross_channel"):
            geo.compress(pts, attributes=[a8, a8], qstep=4, cross_channel=True, **{name: 100})
    with pytest.raises(ValueError, match="choose one of the two"):
        geo.compress(pts, attributes=[a8, a8], qstep=4, target_bytes=100, target_frame_bytes=100)
    check = GeometryCodec._check_rate
    assert check(None, None, 2, 0, None) == (None, False)
    assert check(100, None, 2, 4, None) == ([100, 100], False) and check(None, (7, np.int64(9)), 2, 1, None) == ([7, 9], True)
    assert check(np.array([3, 4]), None, 2, 1, None) == ([3, 4], False)
