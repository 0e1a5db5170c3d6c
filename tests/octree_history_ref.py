"""The reference of compress(..., predict="previous", history=K) (include/pcc.h has the window rule): a predicted
frame is octree_inter_ref's version-4 blob of the frame against the UNION of its window's frames, with the number of
those frames - 1 in byte 3 of the head.  Plain Python / numpy, written from the rule."""
import numpy as np

import octree_inter_ref as ref4

MAX_WINDOW = 8


def union(refs, bias=ref4.BIAS):
    """the distinct points of the frames `refs`, as a Reference"""
    return ref4.Reference(np.concatenate([np.asarray(r, dtype=np.int64).reshape(-1, 3) for r in refs]), bias)


def encode_window(points, refs, bias=ref4.BIAS):
    """the blob of `points` coded against the frames `refs` (1 .. 8 of them, oldest first)"""
    assert 1 <= len(refs) <= MAX_WINDOW
    blob = bytearray(ref4.encode(points, union(refs, bias), bias))
    blob[3] = len(refs) - 1
    return bytes(blob)


def decode_window(blob, refs, bias=ref4.BIAS):
    """version-4 blob -> points, against the last blob[3] + 1 of the frames `refs` (oldest first)"""
    w = blob[3] + 1
    if w > len(refs):
        raise ValueError(f"needs {w} frames in front of it, {len(refs)} are here")
    return ref4.decode(blob, union(refs[len(refs) - w:], bias), bias)


def windows(sizes, history, intra_period=0, n_ref_frames=0):
    """the rule: sizes = the point counts of all frames of a call (the n_ref_frames reference frames first) -> for
    every coded frame None (a frame without points), 0 (intra: version 2) or W, the frames of its window"""
    out, intra = [], set()
    for f in range(n_ref_frames, len(sizes)):
        g = f - n_ref_frames
        if sizes[f] == 0:
            out.append(None)
            continue
        is_intra = (g % intra_period == 0) if intra_period > 0 else f == 0
        if is_intra or f == 0 or sizes[f - 1] == 0:
            intra.add(f)
            out.append(0)
            continue
        w = 1
        while w < history and (f - w) not in intra and f - w - 1 >= 0 and sizes[f - w - 1] > 0:
            w += 1
        out.append(w)
    return out


def encode_chain(frames, history, intra_period=0, references=(), v2=None, bias=ref4.BIAS, cache=None):
    """the blobs of a call: v2(points) writes an intra frame (None: such a frame gives None); cache: a dict that keeps
    blobs by (frame index among references + frames, W) across calls on the same frames"""
    every = [np.asarray(a).reshape(-1, 3) for a in list(references) + list(frames)]
    sizes = [len(np.unique(a, axis=0)) if len(a) else 0 for a in every]
    out = []
    for g, w in enumerate(windows(sizes, history, intra_period, len(references))):
        f = g + len(references)
        if w is None or w == 0:
            out.append(v2(every[f]) if v2 is not None else None)
            continue
        key = (f, w)
        if cache is None or key not in cache:
            blob = encode_window(every[f], every[f - w:f], bias)
            if cache is None:
                out.append(blob)
                continue
            cache[key] = blob
        out.append(cache[key])
    return out
