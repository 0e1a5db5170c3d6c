"""Transform-coded attributes under a byte target (include/pcc.h, "Versions 19 and 21 under a byte target per frame"),
restated in numpy: the ladder of steps, the search over the lengths of the blobs that the existing restatements write
(tests/attr_transform_ref.py for version 19, tests/attr_colour_ref.py for version 21), and the blob the search ends at.
No blob format of its own: what it returns is a blob of one of those two.

  ladder(q, c, bpv)                      the J rungs, each a tuple of c steps
  stage1(J)                              the rungs A = { j : j % 4 == 0 } and J - 1
  choose(length, J, target)              the search; length(j) is asked for the rungs the procedure visits, in its order
  encode(points, values, bpv, q, target, colour=None, bias=32768)   -> (blob, rung, visited rungs)
"""
import numpy as np

import attr_colour_ref
import attr_transform_ref

MUL = (16, 19, 23, 27)     # quarter octaves, in sixteenths


def ladder(q, c, bpv):
    assert bpv in (1, 2) and 1 <= c <= 4, "c = %r, bpv = %r" % (c, bpv)
    top = (1 << (8 * bpv - 1)) - 1
    q = [q] * c if isinstance(q, (int, np.integer)) else list(q)
    assert len(q) == c, "%d steps for %d channels" % (len(q), c)
    for s in q:
        assert isinstance(s, (int, np.integer)) and 1 <= s <= top, "qstep %r with %d bytes per value" % (s, bpv)
    rungs, j = [], 0
    while True:
        rungs.append(tuple(min(top, ((int(s) * MUL[j % 4]) << (j // 4)) >> 4) for s in q))
        if all(s == top for s in rungs[-1]):
            return rungs
        j += 1


def stage1(J):
    return sorted(set(range(0, J, 4)) | {J - 1})


def choose(length, J, target):
    """-> (rung, visited): the rung the frame gets and the rungs whose length was asked for, in order"""
    A, seen = stage1(J), []

    def fits(j):
        seen.append(j)
        return length(j) <= target
    at = next((k for k, a in enumerate(A) if fits(a)), None)
    if at is None:
        return J - 1, seen                       # over its target
    if at == 0:
        return 0, seen
    for j in range(A[at - 1] + 1, A[at]):
        if fits(j):
            return j, seen
    return A[at], seen


def encode_at(points, values, bpv, steps, colour=None, bias=32768):
    """the existing call's blob at the steps of a rung: version 19 for an integer base step without colour (colour is
    None), version 21 otherwise (colour 0 or 1)"""
    if colour is None:
        return attr_transform_ref.encode(points, values, bpv, int(steps[0]), bias)
    return attr_colour_ref.encode(points, values, bpv, tuple(int(s) for s in steps), colour, bias)


def encode(points, values, bpv, q, target, colour=None, bias=32768):
    """q an integer with colour None: version 19; otherwise version 21 (colour 0 or 1)"""
    v = np.asarray(values)
    v = v.reshape(v.shape[0], -1)
    assert isinstance(target, (int, np.integer)) and target >= 1, "target %r" % (target,)
    assert colour is not None or isinstance(q, (int, np.integer)), "a sequence of steps is version 21: colour 0 or 1"
    rungs = ladder(q, v.shape[1], bpv)
    if v.shape[0] == 0:
        return encode_at(points, values, bpv, rungs[0], colour, bias), -1, []
    blobs = {}

    def length(j):
        blobs[j] = encode_at(points, values, bpv, rungs[j], colour, bias)
        return len(blobs[j])
    rung, seen = choose(length, len(rungs), target)
    return blobs[rung], rung, seen
