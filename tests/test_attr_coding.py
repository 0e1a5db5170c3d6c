"""The attribute settings of a call as one record (runtime.AttrCoding), on the CPU: which C entry point a record reaches
and with which arguments, and what GeometryCodec._attr_coding makes of compress's keywords.

Neither test touches the library or a GPU: the first puts a stub in place of the ctypes library, the second is pure
Python.  Every expectation was recorded on the commit before the record existed: the calls below with this stub, the
grid of tests/golden/attr_settings.json by tools/record_attr_settings.py.  Neither is taken from the tree under test.
"""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from conftest import pkg


# ------------------------------------------------------------------ which entry point, with which arguments
class Stub:
    """stands in for the ctypes library: every name is looked up in _abi.PROTOTYPES, the argument count is held to the
    prototype, .calls holds (name, number, ...) as test_geometry_calls.Recorder does, .arrays the ctypes integer arrays
    of the same call as lists; every call returns 0 and writes nothing"""

    def __init__(self):
        self._protos, self.calls, self.arrays = pkg("_abi").PROTOTYPES, [], []

    def __getattr__(self, name):
        kinds = self._protos[name][1]

        def call(*args):
            assert len(args) == len(kinds), (name, len(args), len(kinds))
            self.calls.append((name,) + tuple(a for a, k in zip(args, kinds) if k is not C.c_void_p and type(a) in (int, float)))
            self.arrays.append([list(a) for a in args if isinstance(a, C.Array)])
            return 0
        return call


def stubbed():
    rt = object.__new__(pkg("runtime").Runtime)
    rt.ctx, rt.lib = None, Stub()
    return rt


# two frames of 3 and 2 points, uint8 x 3: values, value offsets, formats, row offsets, points, perm, run starts, n_unique
BASE = (None, [0, 16], [1 | (3 << 8)] * 2, [0, 3, 5], [3, 2], None, None, 5)
# the arrays every call begins with (value offsets, formats, row offsets, points) and ends with (the blobs' offsets)
HEAD, OFFS = [[0, 16], [769, 769], [0, 3, 5], [3, 2]], [[0, 0, 0]]

# keywords of attr_encode_frames -> (the call, its arrays between HEAD and OFFS)
CALLS = [
    ({}, ("pcc_attr_encode_frames", 2, 5, 2408), []),
    (dict(version=2), ("pcc_attr_encode_frames_v2", 2, 5, 0, 2408), []),
    (dict(n_kept=4), ("pcc_attr_encode_frames_kept", 1, 2, 5, 4, 0, 2408), []),
    (dict(version=2, max_error=1), ("pcc_attr_encode_frames_nl", 2, 2, 5, -1, 0, 1, 2408), []),
    (dict(cross=[3, 0]), ("pcc_attr_encode_frames_cross", 1, 2, 5, -1, 0, 0, 2408), [[3, 0]]),
    (dict(cross=[0, 0]), ("pcc_attr_encode_frames", 2, 5, 2408), []),
    (dict(qstep=8), ("pcc_attr_encode_frames_transform", 2, 5, -1, 0, 8, 2408), []),
    (dict(qstep=[4, 8, 8]), ("pcc_attr_encode_frames_transform2", 2, 5, -1, 0, 0, 2408), [[4, 8, 8, 0]]),
    (dict(qstep=8, colour=1), ("pcc_attr_encode_frames_transform2", 2, 5, -1, 0, 1, 2408), [[8, 8, 8, 8]]),
    (dict(qstep=8, scalable_to=2), ("pcc_attr_encode_frames_transform3", 2, 5, -1, 0, 0, 2, 2408), [[8, 8, 8, 8]]),
    (dict(qstep=8, cross=[0, 0], n_kept=4), ("pcc_attr_encode_frames_transform", 2, 5, 4, 0, 8, 2408), []),
]


def test_the_entry_point_of_every_kind_of_call():
    for kw, call, arrays in CALLS:
        rt = stubbed()
        assert rt.attr_encode_frames(*BASE, **kw) == [b"", b""], kw
        assert rt.lib.calls == [call], kw
        assert rt.lib.arrays == [HEAD + arrays + OFFS], kw
    # under a byte target: keys, key_shift, n_kept, qstep, colour, targets
    rt = stubbed()
    assert rt.attr_encode_frames_rate(*BASE, None, 0, None, [4, 8, 8], 1, [100, 200]) == ([b"", b""], [0, 0])
    assert rt.lib.calls == [("pcc_attr_encode_frames_rate", 2, 5, -1, 0, 1, 1, 0, 2408)]
    assert rt.lib.arrays == [HEAD + [[4, 8, 8, 0], [100, 200]] + OFFS + [[0, 0]]]
    rt = stubbed()      # one integer step and no colour: version 19's, and the room and the scratch the caller names
    assert rt.attr_encode_frames_rate(*BASE, None, 6, 4, 8, None, [100, 200], 4096, cap=999) == ([b"", b""], [0, 0])
    assert rt.lib.calls == [("pcc_attr_encode_frames_rate", 2, 5, 4, 6, 0, 0, 4096, 999)]
    assert rt.lib.arrays == [HEAD + [[8, 8, 8, 8], [100, 200]] + OFFS + [[0, 0]]]


def test_refusals():
    rt = stubbed()
    for kw, text in ((dict(version=3), "attribute blob version 3: 1 or 2"),
                     (dict(scalable_to=2, qstep=0), "scalable_to (attribute blob version 22) needs qstep"),
                     (dict(qstep=[1, 2, 3, 4, 5]), "attribute blob version 21: 5 steps, at most 4"),
                     (dict(qstep=8, max_error=1), "qstep (attribute blob versions 19 and 21) has no near-lossless and no cross-channel form"),
                     (dict(cross=[1, 1, 1]), "3 cross-channel masks for 2 frames")):
        with pytest.raises(ValueError) as e:
            rt.attr_encode_frames(*BASE, **kw)
        assert str(e.value) == text
    for qstep, targets, text in ((8, [100], "1 targets for 2 frames"), ([1, 2, 3, 4, 5], [100, 200], "attribute blob version 21: 5 steps, at most 4")):
        with pytest.raises(ValueError) as e:
            rt.attr_encode_frames_rate(*BASE, None, 0, None, qstep, None, targets)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        pkg("runtime").Runtime.attr_rate_ladder([1, 2, 3, 4, 5], 1, 3)
    assert str(e.value) == "5 steps, at most 4"
    assert rt.lib.calls == []


# ------------------------------------------------------------------ what compress makes of its keywords
def test_the_settings_of_compress():
    """1024 rows of keywords -> the exception compress raises, or the settings that reach the attribute coder"""
    G, AttrCoding = pkg("geometry").GeometryCodec, pkg("runtime").AttrCoding
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attr_settings.json")) as f:
        golden = json.load(f)
    axes, rows = golden["axes"], golden["rows"]
    grid = list(itertools.product(*axes.values()))
    assert len(grid) == len(rows) == 1024
    frames = [np.zeros((3, 3), np.int32)] * 2
    values = 0
    for row, want in zip(grid, rows):
        kw = dict(zip(axes, row))
        kw.update(kw.pop("target"))
        attrs = G._check_attributes(frames, [np.zeros((3, 3), np.uint8)] * 2) if kw.pop("attributes") else None
        args = (attrs, len(frames), golden["lod"], kw["scalable"], kw["max_error"], kw["cross_channel"], kw["qstep"], kw["colour"],
                kw["scalable_to"], kw.get("target_bytes"), kw.get("target_frame_bytes"))
        if "error" in want:
            with pytest.raises((TypeError, ValueError)) as e:
                G._attr_coding(*args)
            assert [type(e.value).__name__, str(e.value)] == want["error"], kw
            continue
        c, s = G._attr_coding(*args), want["settings"]
        assert (c is not None) == (attrs is not None) == s["attributes"], kw
        assert s["whole"] == ("target_frame_bytes" in kw), kw      # compress's side: what the geometry blob leaves
        if c is None:
            continue
        values += 1
        assert isinstance(c, AttrCoding) and c.scratch_limit == 0      # the codec's, which compress adds under a target
        steps = None if c.steps is None else list(c.steps) if c.per_channel else [c.steps[0]]
        got = {"attributes": True, "version": c.version, "max_error": c.max_error, "masks": None if c.cross is None else list(c.cross),
               "steps": steps, "per_channel": c.per_channel, "colour": c.colour, "K": c.scalable_to,
               "targets": None if c.targets is None else list(c.targets), "whole": s["whole"]}
        assert got == s, kw
        assert c.steps is None or c.per_channel or set(c.steps) == {c.steps[0]}      # version 19: the one step, for every channel
    assert values == 24
