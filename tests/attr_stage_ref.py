"""The attribute staging rule of include/pcc.h (pcc_attr_stage_frames) restated in numpy.

Integer sources (uint8, uint16) are taken as they are; a uint8 value in a uint16 destination is zero-extended.
Float sources (float32, float64) are quantised with a scale s, per value, in the source's own precision:

    v = clip(rint(x * dtype(s)), 0, peak),      peak = 255 (uint8) or 65535 (uint16)

one IEEE multiplication, round-half-to-even, the clamp on the float before it becomes an integer.  s is narrowed to
float32 once for float32 sources and used as a double for float64 sources.  -0.0 and denormals give 0.  A non-finite
value (NaN, +-Inf) is an error; its output is unspecified, and `quantise` refuses it.  s is not written into any blob.
"""
import numpy as np

KINDS = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}


def quantise(x, s, dtype):
    """float32 / float64 values -> `dtype` (uint8 or uint16) under the rule"""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
    peak = np.iinfo(dtype).max
    with np.errstate(over="ignore"):      # a finite x whose product overflows is clamped like any other
        return np.clip(np.rint(x * x.dtype.type(s)), 0, peak).astype(dtype)


def stage(a, s=None, dtype=None):
    """one frame's attributes [n] or [n, c] -> the uint8 / uint16 [n, c] array the codec codes"""
    a = np.asarray(a)
    a = a[:, None] if a.ndim == 1 else a
    if a.dtype in (np.uint8, np.uint16):
        return np.ascontiguousarray(a if dtype is None else a.astype(dtype))
    if dtype is None:
        dtype = np.uint8 if s <= 255 else np.uint16
    return quantise(a, s, dtype)


def packed(frames, s=None, dtype=None):
    """packed mode: (bytes, offsets) — frame f tight as [rows_f, c_f] of its own width at offsets[f], 16-aligned; the
    pad bytes are 0xEE here, a canary: the kernel does not write them"""
    staged = [stage(a, s, dtype) if np.asarray(a).dtype.kind == "f" else stage(a) for a in frames]      # integers keep their width
    offs, at = [], 0
    for v in staged:
        offs.append(at)
        at += (v.nbytes + 15) // 16 * 16
    out = np.full(at, 0xEE, np.uint8)
    for o, v in zip(offs, staged):
        out[o:o + v.nbytes] = v.reshape(-1).view(np.uint8)
    return out, offs


def sorted_rows(frames, perm, dtype, channels, s=None):
    """sorted mode: [n, channels] of `dtype`, row i = source row perm[i] of the call, absent channels 0; a perm entry
    outside the call gives a zero row"""
    n = sum(np.asarray(a).shape[0] for a in frames)
    rows = np.zeros((n, channels), dtype)
    at = 0
    for a in frames:
        v = stage(a, s, dtype)
        rows[at:at + v.shape[0], :v.shape[1]] = v
        at += v.shape[0]
    perm = np.asarray(perm, np.int64)
    out = np.zeros((perm.shape[0], channels), dtype)
    ok = perm < n
    out[ok] = rows[perm[ok]]
    return out
