"""Attribute transfer onto another geometry (GeometryCodec.transfer, pcc_attr_transfer_frames): the restatement of the
rule (tests/transfer_ref.py) worked by hand and against a second implementation in plain loops, and the ABI.  No GPU;
tests/test_geometry_transfer_gpu.py holds the device to the restatement bit for bit.
"""
import ctypes as C
import os

import numpy as np

import nn_ref
import transfer_ref
from conftest import ROOT, pkg


def test_restatement_hand_worked():
    """Everything on the x axis, y = z = 0, x >= 0: Morton order is x order.

    source rows, as they come (x: value):  39: 50,  21: 7,  3: 1,  0: 2,  6: 100,  21: 10
    targets (rows 0 .. 4):                 x = 1, 5, 20, 30, 40
    distinct source points (rows 0 .. 4):  x = 0, 3, 6, 21, 39; merged values 2, 1, 100, (7 + 10 + 1) // 2 = 9, 50

    backward:  39 -> 40 (distance 1; 30 is at 9)          row 4
               21 -> 20 (1; 30 at 9), both rows           row 2
               3  -> 1 or 5, both at distance 2: a tie, the smaller row wins      row 0
               0  -> 1                                    row 0
               6  -> 5                                    row 1
    so cnt = (2, 1, 2, 0, 1) and
      target 1:  values 1 and 2: (3 + 1) // 2 = 2 — the half rounds up.  Had the tie gone to 5, this were 2 alone
                 and target 5 (1 + 100 + 1) // 2 = 51.
      target 5:  100
      target 20: values 7 and 10: (17 + 1) // 2 = 9
      target 30: nobody's nearest target.  Forward: 21 and 39 are both at distance 9, a tie; 21 is the smaller row (3)
                 of the distinct source points — a duplicated point, whose merged value is 9.  Had the tie gone to 39,
                 this were 50.
      target 40: 50
    """
    src, values, targets, out, cnt = transfer_ref.hand_worked()
    assert src.shape == (6, 3) and targets.shape == (5, 3)
    _, b = nn_ref.nn(src, targets)
    assert b.tolist() == [4, 2, 0, 0, 1, 2]
    distinct, mv = transfer_ref.merged(src, values)
    assert distinct[:, 0].tolist() == [0, 3, 6, 21, 39] and mv[:, 0].tolist() == [2, 1, 100, 9, 50]
    d2, f = nn_ref.nn(targets, distinct)
    assert f.tolist() == [0, 2, 3, 3, 4] and d2.tolist() == [1, 1, 1, 81, 1]
    got, got_cnt = transfer_ref.transfer(src, values, targets)
    assert got.dtype == np.uint8 and got.shape == (5, 1) and got_cnt.dtype == np.uint32
    assert got[:, 0].tolist() == out.tolist() == [2, 100, 9, 9, 50]
    assert got_cnt.tolist() == cnt.tolist() == [2, 1, 2, 0, 1]
    # rows of the target as given: any order, duplicates share their point's value; 1-D values give 1-D back
    rows = targets[[3, 0, 3, 4, 1, 2, 0]]
    got, got_cnt = transfer_ref.transfer_rows(src, values, rows)
    assert got.shape == (7,) and got.tolist() == [9, 2, 9, 50, 100, 9, 2] and got_cnt.tolist() == [0, 2, 0, 1, 1, 2, 2]
    # no source: value 0 and count 0; no target: nothing
    got, got_cnt = transfer_ref.transfer(np.zeros((0, 3)), np.zeros((0, 2), np.uint16), targets)
    assert got.shape == (5, 2) and got.dtype == np.uint16 and not got.any() and not got_cnt.any()
    got, got_cnt = transfer_ref.transfer(src, values, np.zeros((0, 3)))
    assert got.shape == (0, 1) and got_cnt.shape == (0,)


def _loops(src, values, targets):
    """the rule in plain loops over Python ints: targets distinct and Morton-ordered"""
    key = lambda p: int(nn_ref.morton_keys(np.asarray([p]))[0])      # noqa: E731
    d2 = lambda p, q: sum((int(a) - int(b)) ** 2 for a, b in zip(p, q))      # noqa: E731
    c = values.shape[1]
    points = {}      # key -> (point, rows)
    for s, p in enumerate(src):
        points.setdefault(key(p), (p, []))[1].append(s)
    distinct = [points[k] for k in sorted(points)]
    assigned = [[] for _ in targets]
    for s, p in enumerate(src):
        best = None
        for t, q in enumerate(targets):
            if best is None or d2(p, q) < best[0]:      # the first among equals stays
                best = (d2(p, q), t)
        assigned[best[1]].append(s)
    out, cnt = [], []
    for t, q in enumerate(targets):
        rows = assigned[t]
        cnt.append(len(rows))
        if not rows:
            best = None
            for p, r in distinct:
                if best is None or d2(p, q) < best[0]:
                    best = (d2(p, q), r)
            rows = best[1]
        out.append([(sum(int(values[s, ch]) for s in rows) + len(rows) // 2) // len(rows) for ch in range(c)])
    return out, cnt


def test_restatement_against_plain_loops():
    """300 random source rows in a 10^3 cube (duplicates among them, some of them fallbacks) onto 150 other points of a
    slightly larger cube: two implementations that share only the Morton key"""
    rng = np.random.default_rng(17)
    src = rng.integers(-5, 5, (300, 3))
    values = rng.integers(0, 65536, (300, 2)).astype(np.uint16)
    targets = nn_ref.morton_sorted_unique(rng.integers(-7, 7, (150, 3)))
    got, cnt = transfer_ref.transfer(src, values, targets)
    want, want_cnt = _loops(src, values, targets)
    assert got.tolist() == want and cnt.tolist() == want_cnt
    assert np.unique(src, axis=0).shape[0] < 300 and min(want_cnt) == 0 and max(want_cnt) > 1
    # a fallback that is a duplicated source point is among them
    distinct, _ = transfer_ref.merged(src, values)
    _, f = nn_ref.nn(targets, distinct)
    runs = np.array([(src == p).all(1).sum() for p in distinct])
    assert ((cnt == 0) & (runs[f] > 1)).any()


def test_transfer_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    name = "pcc_attr_transfer_frames"
    assert name + "(" in text and name in abi.PROTOTYPES
    res, args = abi.PROTOTYPES[name]
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert res is i32 and args == [vp, vp, i64, vp, i64, vp, vp, vp, i64, i32, i32, i32, vp, vp]
    fn = getattr(abi.lib(), name)
    assert fn.restype is i32 and list(fn.argtypes) == args
    assert abi.lib().pcc_abi_version() == 1
    for word in ("(sum over s in B(t) of v[s] + cnt / 2) / cnt", "nearest DISTINCT source point", "runs no search"):
        assert word in text, word
    # refused without touching a device: no context
    assert fn(None, None, 0, None, 0, None, None, None, 0, 1, 1, 1, None, None) != 0
    assert b"pcc_attr_transfer_frames: bad argument" in abi.lib().pcc_last_error()
