#!/usr/bin/env python3
"""Writes tests/golden/attr_settings.json: what GeometryCodec.compress makes of its attribute keywords, over a grid.

Run once, on the commit before the attribute settings of a call became one record (runtime.AttrCoding): `settle` below
is that commit's check sequence in compress, call for call, over the _check_* methods, which are older than it and
stay.  tests/test_attr_coding.py holds GeometryCodec._attr_coding to the file and never writes it.  Pure Python: no
GPU, no library.

    python tools/record_attr_settings.py            # -> tests/golden/attr_settings.json
"""
import importlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = importlib.import_module("demo-learned-point-cloud-compression_amd.geometry").GeometryCodec

AXES = {
    "scalable": [False, True],
    "max_error": [0, 1],
    "cross_channel": [False, True],
    "qstep": [0, 8, (4, 8, 8), (4, 8)],
    "colour": [None, "ycocg"],
    "scalable_to": [None, 2],
    "target": [{}, {"target_bytes": 100}, {"target_frame_bytes": 100}, {"target_bytes": 100, "target_frame_bytes": 100}],
    "attributes": [False, True],
}
LOD = 0


def grid():
    """the rows of the file, in its order: one dict of compress keywords per row"""
    for row in itertools.product(*AXES.values()):
        kw = dict(zip(AXES, row))
        kw.update(kw.pop("target"))
        yield kw


def frames_of(kw):
    """(frames, attributes) of a row: two frames of three points, uint8 [3, 3] attributes or None"""
    frames = [np.zeros((3, 3), np.int32)] * 2
    return frames, ([np.zeros((3, 3), np.uint8)] * 2 if kw["attributes"] else None)


def settle(kw):
    """the keywords of a row -> the settings that travel to the attribute coder"""
    frames, attributes = frames_of(kw)
    scalable, lod = kw["scalable"], LOD
    version = 2 if scalable else 1
    attrs = None if attributes is None else G._check_attributes(frames, attributes)
    max_error = G._check_max_error(kw["max_error"], attrs)
    cross = G._check_cross(kw["cross_channel"], attrs)
    qstep, steps, colour = G._check_colour(kw["qstep"], kw["colour"], attrs, max_error, scalable, cross)
    steps, scalable_to = G._check_scalable_to(kw["scalable_to"], lod, qstep, steps, attrs, max_error, scalable, cross)
    targets, whole = G._check_rate(kw.get("target_bytes"), kw.get("target_frame_bytes"), len(frames), qstep, scalable_to)
    per_channel = steps is not None      # versions 21 and 22; else the one integer step of version 19, or none
    if steps is None:
        steps = [qstep] if qstep else None
    return {"attributes": attrs is not None, "version": version, "max_error": max_error, "masks": cross, "steps": steps,
            "per_channel": per_channel, "colour": colour, "K": scalable_to, "targets": targets, "whole": whole}


def main():
    rows = []
    for kw in grid():
        try:
            rows.append({"settings": settle(kw)})
        except (TypeError, ValueError) as e:
            rows.append({"error": [type(e).__name__, str(e)]})
    path = os.path.join(ROOT, "tests", "golden", "attr_settings.json")
    with open(path, "w") as f:
        json.dump({"axes": {k: v for k, v in AXES.items()}, "lod": LOD, "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(path, len(rows), "rows,", sum("error" in r for r in rows), "refusals")


if __name__ == "__main__":
    main()
