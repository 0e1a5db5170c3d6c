"""GeometryCodec: lossless geometry-only coding of sequences of point sets (LiDAR sweeps) on the GPU.

Every frame becomes an independent blob of version 2 (csrc/octree2.hip), byte-identical to what the one-frame coder
(pcc_octree_encode_version, version 2) writes for np.unique(points, axis=0) of that frame alone; all frames of a call
are coded side by side by one pcc_octree_encode_frames call and decoded by one pcc_octree_decode_frames call.

    codec = GeometryCodec()
    blobs = codec.compress([pts0, pts1, ...])            # int16 / int32 [n_f, 3] in [-32768, 32767]
    frames = codec.decompress(blobs)                     # int32 [n_f, 3], Morton order (as pcc_octree_decode_dev)
    frames = codec.decompress(blobs, output="device")    # the same as views of one device tensor

    blobs, attr_blobs = codec.compress(frames, attributes=[a0, a1, ...])   # uint8 / uint16 [n_f] or [n_f, c], c <= 4
    frames, attrs = codec.decompress(blobs, attr_blobs)  # attrs[f]: [n_f, c] in its dtype, row i = point i

Levels of detail (csrc/octree2_blob.h has the rule): a stored blob holds every coarser level as a prefix of its bytes.

    nbytes, cells = GeometryCodec.lod_info(blob, 2)      # host only: what a server publishes as a byte range
    cells = codec.decompress([b[:nbytes]], lod=2)        # int32 [cells, 3]: the distinct points >> 2, Morton order
    blobs = codec.compress(frames, lod=2)                # the sender's side: blobs of those cells themselves

Inter-frame prediction (octree blob version 4, csrc/octree4.hip; include/pcc.h has the rule): a frame coded against
the frame before it — every context of version 2 split in three by whether the previous frame has points in the
node's cube and in the child's — about a fifth shorter for consecutive LiDAR sweeps (DESIGN.md 6c has the figures).
A predicted frame decodes level by level and only behind its reference, so a chain decodes frame after frame.

    blobs = codec.compress(frames, predict="previous")                     # frame 0 intra (version 2), the others predicted
    blobs = codec.compress(frames, predict="previous", intra_period=10)    # frames 0, 10, 20, .. are random-access points
    GeometryCodec.geometry_info(blobs[1])      # {"version": 4, "points": n, "predicted": True, "reference_points": n_0}; host only
    frames = codec.decompress(blobs)                                       # any mix of versions 2 and 4
    (b,) = codec.compress([pts_t], predict="previous", reference=pts_t_minus_1)    # a streaming sender: one frame per call
    (pts_t,) = codec.decompress([b], reference=pts_t_minus_1)              # the receiver keeps its last decoded frame

history=K (1 .. 8) codes a predicted frame against the UNION of the up to K frames in front of it (not past an intra
frame or a frame without points): the same blob version against a larger reference, byte 3 of the blob holds the
number of frames - 1, so a decoder needs no keyword.  On 64 x 1800 sweeps K = 4 takes a further 13 % off a
predicted frame with the sensor at rest, 10 % at 10 m/s; the unions are formed on the device by a merge of the frames' sorted keys.

    blobs = codec.compress(frames, predict="previous", history=3)
    GeometryCodec.reference_frames(blobs[3])   # 3: how many decoded frames the blob's reference is the union of; host only
    (b,) = codec.compress([f2], predict="previous", history=2, reference=[f0, f1])     # streaming: the last K frames, oldest first
    (f2,) = codec.decompress([b], reference=[f0, f1])

Predicted frames keep their levels of detail: lod_info answers for version 4 too, and a prefix decodes against the
CELLS of the frames in front of it (a cube above the cut is a union of whole cells), never touching the deep levels.

    cut = [b[:GeometryCodec.lod_info(b, 2)[0]] for b in blobs]             # a chain I P P .., every blob cut at lod 2
    cells = codec.decompress(cut, lod=2)                                   # what version 2's prefixes give
    (c_t,) = codec.decompress([cut[t]], lod=2, reference=c_t_minus_1, reference_lod=2)   # streaming: the cells of before
    (c_t,) = codec.decompress([cut[t]], lod=2, reference=pts_t_minus_1, reference_lod=0) # or lattice points

predict="best" writes every frame as the SHORTEST of its candidates (include/pcc.h has the rule): its version-2 blob
and its version-4 blobs against the windows 1 .. what history=K gives it; of equal lengths version 2, then the smaller
window.  Recorded camera frames mostly stay version 2, LiDAR sweeps take a window, and a sender need not guess.  Every
blob is byte for byte one that predict=None or predict="previous" writes, so decompress, geometry_info,
reference_frames and lod_info take the sequence as it is.  The random-access points are the SCHEDULED intra frames
(frame 0, intra_period): a version-2 blob chosen for its length decodes alone, but a frame behind it may reach past it.

    blobs = codec.compress(frames, predict="best", history=4)              # intra_period, reference as under "previous"
    [GeometryCodec.reference_frames(b) for b in blobs]                     # 0 = version 2, W = the window chosen

Not built: motion compensation, prediction of attributes (they see only the decoded Morton order and are coded as
before).

Attributes are lossless (attribute blob version 1, csrc/attr.hip), one blob per frame beside its geometry blob; the
values of duplicate points merge to their rounded mean per channel, (sum + cnt // 2) // cnt.

Attributes at a level of detail (attribute blob version 2, csrc/attr_blob.h has the rule): the sender chooses it, and
the values of every coarser level are a prefix of that blob's bytes too.

    blobs, attr_blobs = codec.compress(frames, attributes=attrs, scalable=True)
    abytes, values = GeometryCodec.attr_lod_info(attr_blob, 2)        # host only; values == lod_info(blob, 2)[1]
    cells, attrs = codec.decompress([b[:nbytes]], [a[:abytes]], lod=2)

Row j of attrs[f] is the value of the Morton-first point of cell j: a SAMPLE of the cell, where the sender's side
compress(frames, attributes=..., lod=2) stores the cell's MEAN.  At lod 0 version 2 returns what version 1 returns.

Near-lossless attributes (attribute blob versions 4 and 7): a quality setting with a guarantee, chosen by the sender:

    blobs, attr_blobs = codec.compress(frames, attributes=attrs, max_error=2)      # scalable=True, lod=k as before
    GeometryCodec.attr_info(attr_blobs[0])["max_error"]                            # 2: host only, what a receiver reads
    frames, attrs = codec.decompress(blobs, attr_blobs)                            # the kind is read from the blob

Cross-channel prediction (attribute blob versions 8, 11, 13, 14, the cross forms of 1, 2, 4, 7; include/pcc.h has the
rule): what a channel would code is coded as its difference to the channel before it.  The sender's choice for
correlated channels such as a camera's RGB, about a fifth off the colour bytes of recorded frames; uncorrelated channels
grow under it.  The decoded values are exactly those of the same call without it, at every level of detail:

    blobs, attr_blobs = codec.compress(frames, attributes=rgb, cross_channel=True)     # with scalable, lod, max_error
    blobs, attr_blobs = codec.compress(frames, attributes=rgbx, cross_channel=(1, 2))  # G against R, B against G, X alone
    GeometryCodec.attr_info(attr_blobs[0])["cross_channel"]                            # (1, 2); absent from a plain kind

No decoded value is off by more than max_error from what max_error=0 (the default, lossless, the bytes of before)
returns for the same call.  include/pcc.h states the rule.

Attributes predicted from 3-D neighbours (attribute blob versions 25 and 26, the second the cross-channel form;
include/pcc.h has the rule): lossless, version 2's layout and prefixes, every value predicted from up to three
Morton-first points of the coarser cells around its point; about a tenth smaller than versions 1 and 2 on colour:

    blobs, attr_blobs = codec.compress(frames, attributes=rgb, predictor="neighbours")   # with lod, cross_channel
    GeometryCodec.attr_info(attr_blobs[0])["predictor"]                                  # "neighbours"; absent from other kinds

Their bounded-error forms (versions 28 and 31): version 7's layout and prefixes, the same candidates in a closed loop over
decoded values, |v - v^| <= max_error; 11 to 25 % smaller than versions 7 and 14 on colour at max_error 1 .. 8:

    blobs, attr_blobs = codec.compress(frames, attributes=rgb, predictor="bounded-neighbours", max_error=2)
    GeometryCodec.attr_info(attr_blobs[0])      # "predictor": "neighbours", "max_error": 2, "scalable": True

Transform-coded attributes (attribute blob versions 19 and 21, include/pcc.h has the rule): lossy, for rates below about
a byte per point.  Version 21 decorrelates colour first (luma and two chroma differences) and gives every channel its own
step: on recorded camera colour it is shorter AND closer at q = 16 than plain RGB at q = 32.

    blobs, attr_blobs = codec.compress(frames, attributes=rgb, qstep=32)                     # version 19: one step, R G B
    blobs, attr_blobs = codec.compress(frames, attributes=rgb, qstep=16, colour="ycocg")     # version 21: Y Co Cg
    blobs, attr_blobs = codec.compress(frames, attributes=rgb, qstep=(16, 32, 32), colour="ycocg")   # coarser chroma
    blobs, attr_blobs = codec.compress(frames, attributes=rgbi, qstep=(8, 8, 8, 40))         # a step per channel, no transform
    GeometryCodec.attr_info(attr_blobs[0])       # version 21: "qstep" a tuple of c steps, "colour" "ycocg" or None

Version 22 is version 21 under weights that a decoder holding only a geometry prefix can form: the sender names its
deepest cut K, and levels of detail 0 .. K are prefixes of the blob, as version 2's are, at a few per cent more bytes
than version 19 at equal error.  Row j at a level is the mean of cell j under the kind's weights.

    blobs, attr_blobs = codec.compress(frames, attributes=rgb, qstep=16, colour="ycocg", scalable_to=3)   # version 22
    abytes, values = GeometryCodec.attr_lod_info(attr_blobs[0], 2)             # host only; lod <= K
    cells, coarse = codec.decompress([b[:GeometryCodec.lod_info(b, 2)[0]] for b in blobs],
                                     [a[:GeometryCodec.attr_lod_info(a, 2)[0]] for a in attr_blobs], lod=2)

A byte budget for versions 19 and 21: qstep is the finest setting the sender accepts, and every frame is coded at the
first coarser one of a quarter-octave ladder that a fixed search (include/pcc.h) finds under its target, in one call.
The blob is the one the plain call writes at those steps; no format and no decoder is new.

    blobs, attr_blobs = codec.compress(frames, attributes=rgb, qstep=(4, 8, 8), colour="ycocg", target_bytes=6000)
    GeometryCodec.attr_info(attr_blobs[0])["qstep"]                            # what the frame got, e.g. (23, 46, 46)
    GeometryCodec.rate_ladder((4, 8, 8), np.uint8)                             # host only: the 21 settings to choose from
    blobs, attr_blobs = codec.compress(frames, attributes=rgb, qstep=8, target_frame_bytes=16000)   # geometry + attributes

Metric frames (include/pcc.h has the rule): float32 points in the caller's unit, from the host or from this codec's
device, are put on the lattice by the codec, q = rint((x - origin) / voxel) per coordinate in float32; rows without a
return (NaN / Inf) can be dropped, and the row index says which decoded row every input row became.

    blobs = codec.compress([xyz0, xyz1, ...], voxel=0.02, invalid="drop")      # float32 [n_f, 3], numpy or torch
    blobs, index = codec.compress(frames, voxel=0.02, return_index=True)       # index[f]: int32 [n_f], -1 = dropped
    frames = codec.decompress(blobs, voxel=0.02)                               # float32 [n_f, 3]: origin + c * voxel

voxel and origin are not written into any blob: the caller carries the grid.

Attributes from where they lie (include/pcc.h has the rule, csrc/attr_stage.hip the kernel): uint8 / uint16 tensors on
this codec's device are read there, and float32 / float64 values, host or device, are quantised on the device,
v = clip(rint(x * s), 0, peak) in their own precision; compress, distortion and transfer take both.

    blobs, attr_blobs = codec.compress(frames, attributes=[t0, t1, ...])       # torch uint8 / uint16 on the codec's device
    blobs, attr_blobs = codec.compress(frames, attributes=[interleaved[:, 4:7]])   # a view with contiguous rows: no copy
    with rt:                                                                   # the capture step's Runtime: its stream is waited for
        f = capture.voxelize(rt, xyzrgba, output="device")                     # int32 points, float64 colours in [0, 1]
        blobs, attr_blobs = codec.compress([f["points"]], attributes=[f["colors"]], attribute_scale=255)
    moved = codec.transfer(frames, attrs, lossy, output="device")              # and on into compress / distortion, on the device
    rep = codec.distortion(frames, frames, normals_a=codec.normals(frames, output="device"))

The scale is not written into any blob either: decompress returns the integers.

Distortion (include/pcc.h has the rule): what a lossy setting costs, as the D1 (point-to-point) figures of MPEG's
pc_error, by exact nearest neighbours on the device; lattice frames from the host or from this codec's device.

    cells = codec.decompress([b[:nbytes]], lod=2)[0]
    rep = codec.distortion([pts], [(cells << 2) + 2], peak=1023)     # rep[0]: mse_ab, mse_ba, max_ab, max_ba, d1_psnr
    rep = codec.distortion(frames, lossy, attributes_a=attrs, attributes_b=lossy_attrs)      # + attr_mse_ab / _ba
    rep = codec.distortion(frames, lossy, normals_a="estimate", peak=1023)      # + d2_mse_ab / _ba, d2_psnr (point-to-plane)

Surface normals (include/pcc.h has the rule): per point the eigenvector of the smallest eigenvalue of the scatter
matrix of its k nearest neighbours, found exactly on the device; for shading, registration and the D2 figures above.

    normals = codec.normals(frames, k=16, viewpoint=(0, 0, 0))      # float32 [n_f, 3] per frame, row i = input row i

Outlier removal (include/pcc.h has both rules): the pre-step of a capture pipeline, on the device — flying pixels and
isolated returns are the most expensive points an octree codes.  Verdicts per frame over its distinct lattice points by
exact k nearest neighbours, decided in integers; the rows returned are the caller's own, in input order.

    kept = codec.filter(frames, method="statistical", k=16, std_ratio=2.0)      # Open3D's remove_statistical_outlier
    kept, attrs = codec.filter(frames, attributes=rgb, method="radius", min_neighbours=4, radius2=9)
    kept, mask, report = codec.filter(frames, return_mask=True, return_report=True, output="device")
    blobs = codec.compress(codec.filter(frames))

Clusters (include/pcc.h has the rule): what a k-NN score cannot see — blobs of flying pixels along a depth edge, a
detached piece of background — by DBSCAN on the device: connected components of the points within a radius of each
other, numbered by size, as a function of the point set alone.

    labels = codec.cluster(frames, radius2=3, min_points=50)      # int32 [n_f] per frame, row i = input row i, noise -1
    subject = [f[l == 0] for f, l in zip(frames, labels)]          # the largest cluster; l >= 0: without small debris
    labels, report = codec.cluster(frames, radius2=3, min_neighbours=4, return_report=True, output="device")

One Runtime (ctx + stream) per codec; calls on the same instance are serialised, instances on different threads run
side by side.
"""
import ctypes as C
import re
import struct
import threading
from typing import NamedTuple

import numpy as np
import torch

from ._abi import check, PccError, PCC_E_ARG, PCC_E_RANGE
from .runtime import Runtime, AttrCoding, _ptr, ATTR_RUN_KINDS, ATTR_TRANSFORM_KINDS, ATTR_SCALABLE_TRANSFORM_KIND, ATTR_SRC_KINDS

MAX_FRAMES = 65535      # the batch-index range of pcc_morton_keys
MAX_HISTORY = 8         # frames a predicted frame's reference may be the union of (kO4MaxWindow, csrc/octree4.h)
MAX_LOD = 15            # levels of detail 0 .. 15 (csrc/octree2_blob.h)


def _ends(sizes):
    """[0, n_0, n_0 + n_1, ...]: where the rows of every frame of a call begin, and behind them the call's total"""
    return np.cumsum([0] + list(sizes)).tolist()


def _split(whole, sizes):
    """the rows of a call, frame behind frame -> one view of `whole` per frame"""
    ends = _ends(sizes)
    return [whole[a:b] for a, b in zip(ends[:-1], ends[1:])]


def _frames_out(rt, whole, sizes, to_host):
    """the rows of a call in one device tensor -> one view per frame: of that tensor, or (to_host) of one pinned host
    copy of it, behind one rt.sync()"""
    if to_host:
        host = torch.empty(whole.shape, dtype=whole.dtype, pin_memory=True)
        host.copy_(whole, non_blocking=True)
        whole = host.numpy()
    rt.sync()      # the host copy is complete; a device result may be read from the caller's stream at once
    return _split(whole, sizes)


class QstepLengthError(ValueError, TypeError):
    """compress(..., qstep=(..)) with another number of steps than a frame has channels.  A ValueError; also a TypeError,
    which every sequence qstep raised before sequences had a meaning, so a caller that caught that still does."""


class _Front(NamedTuple):
    """What the front end of a call (GeometryCodec._front: stage, keys, sorted / distinct) hands to compress and to
    distortion.  Nothing to code (n_keep == 0): the fields behind n_keep stay at their defaults."""
    nb: int                      # frames
    sizes: list                  # input rows per frame
    n: int                       # input rows of the call
    n_keep: int                  # rows that were not dropped: the sorted keys in front of the dropped rows' keys
    offsets: object = None       # the upload, the int64 frame offsets first: rows_index reads them on the device
    perm: object = None          # sort_pairs' permutation of all n keys
    sorted_keys: object = None   # the n_keep sorted keys with their duplicates, under the lod mask
    rows: object = None          # pcc_unique_rows: the first row of every run of equal keys
    n_unique: int = 0
    keys: object = None          # the distinct keys (sorted_keys itself where there is no duplicate)


class _Attr(NamedTuple):
    """A frame's attributes that reach the coders through pcc_attr_stage_frames (include/pcc.h has the rule): a tensor on
    the codec's device, or a host float array.  shape, dtype and nbytes answer as the uint8 / uint16 array it becomes."""
    src: object      # [n, c]: a device tensor whose rows lie `pitch` elements apart, or a C-contiguous host array
    kind: int        # ATTR_SRC_KINDS: what a value of src is
    pitch: int
    shape: tuple     # (n, c)
    dtype: object    # the numpy dtype of the values after staging

    @property
    def nbytes(self):
        return self.shape[0] * self.shape[1] * self.dtype.itemsize

    @property
    def on_device(self):
        return isinstance(self.src, torch.Tensor)


class GeometryCodec:
    def __init__(self, device=0):
        self.rt = Runtime(device)
        self._lock = threading.Lock()
        self.rate_scratch_limit = 0      # bytes of scratch a budgeted compress may take for its candidate rows; 0: the library's default

    def close(self):
        self.rt.close()

    @property
    def _device(self):
        """this codec's device; None for an instance without a Runtime (the keyword checks run without one)"""
        rt = getattr(self, "rt", None)
        return None if rt is None else rt.device

    def _check_frames(self, frames):
        """-> (frames, is_float, on_device): numpy arrays (host) or tensors on this codec's device, all integer (int16 /
        int32) or all float32"""
        out, kinds, places = [], [], []
        for f, a in enumerate(frames):
            if isinstance(a, torch.Tensor):
                if a.device.type == "cpu":
                    a = a.detach().numpy()
                elif a.device != self.rt.device:
                    raise ValueError(f"frame {f}: a tensor on {a.device}, this codec runs on {self.rt.device}")
            else:
                a = np.asarray(a)
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"frame {f}: expected an [n, 3] array, got shape {tuple(a.shape)}")
            name = str(a.dtype).replace("torch.", "")
            if name == "float32":
                kinds.append(True)
            elif name in ("int16", "int32"):
                kinds.append(False)
            elif name == "float64":
                raise TypeError(f"frame {f}: float64 coordinates are not narrowed silently; pass float32 (with voxel=), "
                                "int16 or int32")
            else:
                raise TypeError(f"frame {f}: expected int16 or int32 coordinates, got {a.dtype}")
            places.append(isinstance(a, torch.Tensor))
            if kinds[-1] != kinds[0]:
                raise ValueError(f"frame {f}: {a.dtype} beside {out[0].dtype} in frame 0: the frames of a call are all "
                                 "integer or all float32")
            if places[-1] != places[0]:
                raise ValueError(f"frame {f}: on the {'device' if places[-1] else 'host'}, frame 0 on the "
                                 f"{'device' if places[0] else 'host'}: the frames of a call are all on the host or all "
                                 "on the device")
            out.append(a)
        if len(out) > MAX_FRAMES:
            raise ValueError(f"{len(out)} frames in one call, at most {MAX_FRAMES}")
        return out, bool(kinds and kinds[0]), bool(places and places[0])

    @staticmethod
    def _check_grid(voxel, origin, what):
        """voxel and origin narrowed to float32 once: (float, (float, float, float)) as the device will use them"""
        try:
            with np.errstate(all="ignore"):
                v = np.float32(voxel)
                o = np.asarray(origin, dtype=np.float32).reshape(-1)
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"{what}: voxel must be a number and origin three numbers, got {voxel!r}, {origin!r}") from None
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{what}: voxel must be a positive finite number (as float32), got {voxel!r}")
        if o.shape != (3,) or not np.isfinite(o).all():
            raise ValueError(f"{what}: origin must be three finite numbers (as float32), got {origin!r}")
        return float(v), tuple(float(x) for x in o)

    @staticmethod
    def _check_output(output):
        if output not in ("numpy", "device"):
            raise ValueError(f"output must be 'numpy' or 'device', got {output!r}")

    @staticmethod
    def _check_invalid(invalid):
        if invalid not in ("raise", "drop"):
            raise ValueError(f"invalid must be 'raise' or 'drop', got {invalid!r}")

    @staticmethod
    def _check_voxel(is_float, voxel, origin, what):
        """the grid of a call that takes lattice or float32 frames -> (voxel, origin): float32 frames need one (as
        _check_grid narrows it), integer frames refuse one"""
        if is_float:
            if voxel is None:
                raise ValueError("float32 frames need voxel=, the edge of a lattice cell in the frames' unit")
            return GeometryCodec._check_grid(voxel, origin, what)
        if voxel is not None:
            raise ValueError("voxel= with integer frames: they are on the lattice already")
        return voxel, origin

    def _check_two_sides(self, frames_a, frames_b, where, hint=""):
        """the frames of both sides of distortion and transfer -> (frames, on_device) of side A, then of side B: lattice
        points, as many frames on one side as on the other, both on the host or both on the device; hint: the call's
        own last words to a caller with float32 frames"""
        fa, float_a, dev_a = self._check_frames(frames_a)
        fb, float_b, dev_b = self._check_frames(frames_b)
        if float_a or float_b:
            raise TypeError(f"{where}: float32 frames: pass lattice points (int16 / int32) — the input of compress, or "
                            f"what decompress returns without voxel={hint}")
        if len(fa) != len(fb):
            raise ValueError(f"{where}: {len(fa)} frames against {len(fb)}")
        if fa and dev_a != dev_b:
            raise ValueError(f"{where}: one side on the host, the other on the device: the frames of a call are all on "
                             "the host or all on the device")
        return fa, dev_a, fb, dev_b

    @staticmethod
    def _common_format(attrs):
        """the common format of a call's attributes -> (dtype, channels): uint16 if any frame is, rows of 4 or 8 bytes
        (pcc_gather_rows), absent channels 0"""
        dtype = np.uint16 if any(a.dtype == np.uint16 for a in attrs) else np.uint8
        channels = max(a.shape[1] for a in attrs)
        return dtype, 4 if dtype == np.uint8 or channels > 2 else 2

    @staticmethod
    def _input_rows(rt, front):
        """the distinct row of every input row of a front end: rows_index with no frame's rows taken off"""
        return rt.rows_index(front.perm, front.n_keep, front.rows, front.n_unique, front.offsets.data_ptr(),
                             torch.zeros(front.nb, dtype=torch.int64, device=rt.device), front.nb)

    @staticmethod
    def _check_attribute_scale(scale, dtype, given):
        """attribute_scale and attribute_dtype of a call -> (s as a float, the numpy dtype float values become), or
        (None, None) without a scale; `given`: whether the call has attributes"""
        if scale is None:
            if dtype is not None:
                raise ValueError("attribute_dtype is what float attributes become: it needs attribute_scale=")
            return None, None
        if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)):
            raise TypeError(f"attribute_scale must be a number, got {scale!r}")
        s = float(scale)
        if not (np.isfinite(s) and 0.0 < s <= 65535.0):
            raise ValueError(f"attribute_scale must be a finite number with 0 < s <= 65535, got {scale!r}")
        if not given:
            raise ValueError("attribute_scale quantises float attributes: it needs attributes")
        if dtype is None:
            return s, np.dtype(np.uint8 if s <= 255.0 else np.uint16)
        try:
            dtype = np.dtype(dtype)
        except TypeError:
            dtype = None
        if dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise ValueError("attribute_dtype must be np.uint8 or np.uint16")
        return s, dtype

    @staticmethod
    def _check_attributes(frames, attributes, device=None, scale=None, dtype=None):
        """-> one entry per frame: host uint8 / uint16 arrays become C-contiguous [n, c] numpy arrays, as before; tensors
        on `device` (the codec's) and float arrays (scale: attribute_scale, dtype: what they become) become _Attr
        records, which reach the device layouts through pcc_attr_stage_frames.  All on the host or all on the device."""
        attributes = list(attributes)
        if len(attributes) != len(frames):
            raise ValueError(f"{len(attributes)} attribute arrays for {len(frames)} frames")
        out, places = [], []
        for f, (a, p) in enumerate(zip(attributes, frames)):
            on_device = False
            if isinstance(a, torch.Tensor) and a.device.type != "cpu":
                if device is None or a.device != device:
                    raise ValueError(f"frame {f}: attributes on {a.device}, this codec runs on {device}")
                on_device, a = True, a.detach()
            elif isinstance(a, torch.Tensor):
                a = a.detach().numpy()
            else:
                a = np.asarray(a)
            name = str(a.dtype).replace("torch.", "")
            if name in ("float32", "float64"):
                if scale is None:
                    raise TypeError(f"frame {f}: expected uint8 or uint16 attributes, got {name}; float values are quantised "
                                    "under attribute_scale=s, v = clip(rint(x * s), 0, peak)")
            elif name not in ("uint8", "uint16"):
                raise TypeError(f"frame {f}: expected uint8 or uint16 attributes, got {name}")
            elif scale is not None:
                raise ValueError(f"frame {f}: attribute_scale with {name} attributes: integer values are taken as they are")
            places.append(on_device)
            if places[-1] != places[0]:
                raise ValueError(f"frame {f}: attributes on the {'device' if places[-1] else 'host'}, frame 0's on the "
                                 f"{'device' if places[0] else 'host'}: the attributes of a call are all on the host or "
                                 "all on the device")
            if a.ndim == 1:
                a = a[:, None]
            if a.ndim != 2 or not 1 <= a.shape[1] <= 4:
                raise ValueError(f"frame {f}: expected attributes of shape [n] or [n, c] with 1 <= c <= 4, got {tuple(a.shape)}")
            if a.shape[0] != p.shape[0]:
                raise ValueError(f"frame {f}: {a.shape[0]} attribute rows for {p.shape[0]} points")
            n, c = int(a.shape[0]), int(a.shape[1])
            if not on_device:
                a = np.ascontiguousarray(a.astype(a.dtype.newbyteorder("<"), copy=False))
                if scale is None:      # host integers: the path and the bytes of before
                    out.append(a)
                    continue
                pitch = c
            else:
                if (c > 1 and a.stride(1) != 1) or (n > 1 and a.stride(0) < c):
                    a = a.contiguous()      # a [:, 4:7] view goes in by its pitch; a transposed or broadcast one is copied
                pitch = max(int(a.stride(0)), c) if n > 1 else c
            out.append(_Attr(a, ATTR_SRC_KINDS[name], pitch, (n, c), np.dtype(name) if scale is None else dtype))
        return out

    @staticmethod
    def _staged(attrs):
        """whether the attributes of a call go through pcc_attr_stage_frames (all or none do)"""
        return bool(attrs) and isinstance(attrs[0], _Attr)

    @staticmethod
    def _stage_attributes(rt, attrs, caller, scale, channels=0, perm=None, dtype=None):
        """_Attr records -> Runtime.attr_stage_frames' result: packed (channels 0) for the coders, or sorted rows of
        `dtype` under the sort's permutation.  Device sources are read behind whatever the caller's stream still does
        to them."""
        if attrs[0].on_device:
            rt.stream.wait_stream(caller)
        bpv = np.dtype(dtype).itemsize if channels else max(a.dtype.itemsize if a.kind >= 2 else 1 for a in attrs)
        return rt.attr_stage_frames([(a.src, a.kind, a.shape[1], a.pitch) for a in attrs], _ends([a.shape[0] for a in attrs]),
                                    1.0 if scale is None else scale, bpv, channels, perm)

    @staticmethod
    def _check_stage_status(status, where):
        """the status word of pcc_attr_stage_frames, read behind a synchronisation the call has had"""
        bits = int(status.item())
        if bits & 1:
            raise PccError(PCC_E_RANGE, f"{where} (pcc_attr_stage_frames)", "non-finite attribute value (NaN or Inf)")
        if bits & 2:
            raise PccError(PCC_E_ARG, f"{where} (pcc_attr_stage_frames)", "a row of the permutation outside the call")

    @staticmethod
    def _check_lod(lod):
        if not isinstance(lod, (int, np.integer)) or isinstance(lod, bool) or not 0 <= lod <= MAX_LOD:
            raise ValueError(f"lod must be an integer in 0 .. {MAX_LOD}, got {lod!r} (32768 is not a multiple of 2^16: "
                             "the cells of level 16 would not nest in a root cube)")
        return int(lod)

    @staticmethod
    def lod_info(blob, lod):
        """(bytes, cells) of level of detail `lod` of a version-2 or version-4 blob: blob[:bytes] is the shortest prefix
        that decompress(..., lod=lod) reads, `cells` the rows it gives.  Host only (no GPU needed); `blob` may be a
        prefix that reaches the last needed chunk's length table (lod 0 of a version-4 blob: the whole blob)."""
        return Runtime.octree_lod_info(bytes(blob), GeometryCodec._check_lod(lod))

    @staticmethod
    def attr_lod_info(attr_blob, lod):
        """(bytes, values) of level of detail `lod` of a version-2 attribute blob (compress(..., scalable=True)), of a
        version-25 / 26 or 28 / 31 blob (compress(..., predictor="neighbours" / "bounded-neighbours")), or of a
        version-22 blob (compress(..., qstep=q, scalable_to=K); lod <= K, PccError above):
        attr_blob[:bytes] is the shortest prefix that decompress(..., lod=lod) reads, `values` the rows it gives (the
        cells of the frame's geometry at that lod).  Host only; `attr_blob` may be a prefix that reaches the last needed
        chunk's length table."""
        return Runtime.attr_lod_info(bytes(attr_blob), GeometryCodec._check_lod(lod))

    @staticmethod
    def attr_info(attr_blob):
        """what the head of an attribute blob of any kind says, as a dict: version (1, 2, 4, 7, their cross-channel
        forms 8, 11, 13, 14, or the transform-coded 19), bpv (bytes per value), channels, points, max_error (0: lossless,
        and version 19; a blob without points records none), scalable, lod (the sender's); a cross-channel kind adds
        cross_channel, the tuple of channel indices coded against the channel before them (a plain kind's dict has no
        such key), version 19 adds qstep (0 in a blob without points), version 21 qstep as a tuple of one step per
        channel and colour, "ycocg" or None (zeros and None in a blob without points), version 22 those two, scalable
        True and scalable_to, its K (0 in a blob without points); versions 25 and 26 add predictor, "neighbours" (no other
        kind's dict has the key), 26 also cross_channel; versions 28 and 31 the same predictor beside their max_error >= 1
        and scalable True, 31 also cross_channel.
        Host only; `attr_blob` may be a prefix of 16 bytes or more (version 21: 16 + 4 channels)."""
        return Runtime.attr_info(bytes(attr_blob))

    @staticmethod
    def _check_max_error(max_error, attrs):
        if isinstance(max_error, bool) or not isinstance(max_error, (int, np.integer)):
            raise TypeError(f"max_error must be an integer >= 0, got {max_error!r}")
        max_error = int(max_error)
        if max_error < 0:
            raise ValueError(f"max_error must be an integer >= 0, got {max_error}")
        if max_error and attrs is None:
            raise ValueError("max_error bounds the error of attributes: it needs attributes=")
        for f, a in enumerate(attrs or ()):
            if max_error >= 1 << (8 * a.dtype.itemsize - 1):
                raise ValueError(f"frame {f}: max_error {max_error} is too large for {a.dtype} attributes, at most "
                                 f"{(1 << (8 * a.dtype.itemsize - 1)) - 1}")
        return max_error

    @staticmethod
    def _check_qstep(qstep, attrs, max_error, scalable, cross):
        if isinstance(qstep, bool) or not isinstance(qstep, (int, np.integer)):
            raise TypeError(f"qstep must be an integer >= 0, got {qstep!r}")
        qstep = int(qstep)
        if qstep < 0:
            raise ValueError(f"qstep must be an integer >= 0, got {qstep}")
        if qstep == 0:
            return 0
        if attrs is None:
            raise ValueError("qstep is the quantiser step of transform-coded attributes: it needs attributes=")
        if max_error:
            raise ValueError("qstep with max_error: a transform-coded blob (version 19) bounds no single value's error; choose "
                             "one of the two")
        if scalable:
            raise ValueError("qstep with scalable=True: a transform-coded blob (version 19) has no level-of-detail prefixes, "
                             "the weights of its transform need every point")
        if cross is not None:
            raise ValueError("qstep with cross_channel: attribute blob version 19 has no cross-channel form")
        for f, a in enumerate(attrs):
            if qstep >= 1 << (8 * a.dtype.itemsize - 1):
                raise ValueError(f"frame {f}: qstep {qstep} is too large for {a.dtype} attributes, at most "
                                 f"{(1 << (8 * a.dtype.itemsize - 1)) - 1}")
        return qstep

    @staticmethod
    def _check_colour(qstep, colour, attrs, max_error, scalable, cross):
        """qstep and colour of compress -> (qstep, steps, colour): steps None and colour 0 for the calls of before (no
        transform-coded blob, or version 19 with its one integer step); else version 21, steps a list of one step per
        channel of the widest frame (an integer qstep serves every channel) and colour 0 or 1"""
        if colour is not None and colour != "ycocg":
            raise ValueError(f"colour must be None or 'ycocg', got {colour!r}")
        if isinstance(qstep, (tuple, list)):
            if any(isinstance(q, bool) or not isinstance(q, (int, np.integer)) for q in qstep):
                raise TypeError(f"qstep must be an integer >= 0 or a sequence of integers >= 1, one per channel, got {qstep!r}")
            steps = [int(q) for q in qstep]
            if attrs is None:
                raise ValueError("qstep is the quantiser step of transform-coded attributes: it needs attributes=")
            for f, a in enumerate(attrs):
                if len(steps) != a.shape[1]:
                    raise QstepLengthError(f"frame {f}: qstep has {len(steps)} steps, the frame has {a.shape[1]} channels")
        else:
            steps = None
        q = GeometryCodec._check_qstep(qstep if steps is None else 1, attrs, max_error, scalable, cross)      # a sequence: what it refuses beside it
        if steps is None and colour is None:
            return q, None, 0
        if steps is None:
            if q == 0:
                raise ValueError("colour='ycocg' is the colour transform of transform-coded attributes: it needs qstep= (the "
                                 "lossless and bounded kinds have cross_channel= for correlated channels)")
            steps = [q] * max(a.shape[1] for a in attrs)
        for f, a in enumerate(attrs):
            top = (1 << (8 * a.dtype.itemsize - 1)) - 1
            for ch, sq in enumerate(steps[:a.shape[1]]):
                if sq < 1 or sq > top:
                    raise ValueError(f"frame {f}: qstep {sq} of channel {ch} is outside 1 .. {top} for {a.dtype} attributes")
            if colour is not None and a.shape[1] < 3:
                raise ValueError(f"frame {f}: colour='ycocg' needs 3 channels (R, G, B), the frame has {a.shape[1]}")
        return 1, steps, int(colour is not None)

    @staticmethod
    def _check_scalable_to(scalable_to, lod, qstep, steps, attrs, max_error, scalable, cross):
        """scalable_to of compress -> (steps, K): None and the steps as they were for the calls of before; else version
        22, K an integer in 1 .. 15 - lod and one step per channel of the widest frame"""
        if scalable_to is None:
            return steps, None
        if isinstance(scalable_to, bool) or not isinstance(scalable_to, (int, np.integer)):
            raise TypeError(f"scalable_to must be an integer in 1 .. {15 - lod}, got {scalable_to!r}")
        K = int(scalable_to)
        if not 1 <= K <= 15 - lod:
            raise ValueError(f"scalable_to must be an integer in 1 .. {15 - lod} (15 - lod), got {K}")
        if max_error or cross is not None or scalable:
            raise ValueError("scalable_to with max_error, cross_channel or scalable=True: it is the deepest level-of-detail prefix "
                             "of transform-coded attributes (qstep=), which have none of the three")
        if not qstep:
            raise ValueError("scalable_to is the deepest level-of-detail prefix of transform-coded attributes: it needs qstep=")
        if steps is None:      # an integer qstep serves every channel, as it does with colour=
            steps = [qstep] * max(a.shape[1] for a in attrs)
        return steps, K

    @staticmethod
    def rate_ladder(qstep, dtype, channels=None):
        """the steps that compress(..., qstep=qstep, target_bytes=B) may choose from, finest first: a list of J tuples
        of one step per channel (include/pcc.h has the rule: quarter octaves from qstep up to the coarsest step of
        `dtype`, uint8 or uint16).  qstep an integer (channels then says how many it serves, default 1) or one step per
        channel.  Host only."""
        bpv = np.dtype(dtype).itemsize
        if np.dtype(dtype) not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise TypeError(f"attributes are uint8 or uint16, got {np.dtype(dtype)}")
        if isinstance(qstep, (tuple, list)):
            if channels is not None and int(channels) != len(qstep):
                raise ValueError(f"qstep has {len(qstep)} steps for {channels} channels")
            channels = len(qstep)
        return Runtime.attr_rate_ladder(qstep, bpv, 1 if channels is None else int(channels))

    @staticmethod
    def _check_rate(target_bytes, target_frame_bytes, nb, qstep, scalable_to):
        """target_bytes / target_frame_bytes of compress -> (one target per frame, whether it bounds geometry and
        attributes together), or (None, False) for the calls of before"""
        if target_bytes is None and target_frame_bytes is None:
            return None, False
        if target_bytes is not None and target_frame_bytes is not None:
            raise ValueError("target_bytes bounds a frame's attribute blob, target_frame_bytes its two blobs together: choose one of the two")
        name, t = ("target_bytes", target_bytes) if target_bytes is not None else ("target_frame_bytes", target_frame_bytes)
        seq = list(t) if isinstance(t, (tuple, list, np.ndarray)) else None
        for v in ([t] if seq is None else seq):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer >= 1 or a sequence of one per frame, got {t!r}")
        if seq is not None and len(seq) != nb:
            raise ValueError(f"{name} has {len(seq)} entries for {nb} frames")
        targets = [int(v) for v in (seq if seq is not None else [t] * nb)]
        for f, v in enumerate(targets):
            if v < 1:
                raise ValueError(f"frame {f}: {name} must be at least 1, got {v}")
        if not qstep:
            raise ValueError(f"{name} chooses the steps of transform-coded attributes from qstep upwards: it needs qstep= (and attributes=)")
        if scalable_to is not None:
            raise ValueError(f"{name} with scalable_to: the lift of attribute blob version 22 has other weights, a byte target "
                             "covers versions 19 and 21 only")
        return targets, target_frame_bytes is not None

    @staticmethod
    def _check_cross(cross_channel, attrs):
        """cross_channel of compress -> one mask per frame (bit ch - 1: channel ch against ch - 1), or None for False"""
        if cross_channel is False:
            return None
        if cross_channel is True:
            chans = None
        elif isinstance(cross_channel, (tuple, list, range)) and all(
                isinstance(ch, (int, np.integer)) and not isinstance(ch, bool) for ch in cross_channel):
            chans = sorted(int(ch) for ch in cross_channel)
            if len(set(chans)) != len(chans) or any(ch < 1 or ch > 3 for ch in chans):
                raise ValueError(f"cross_channel must name distinct channels in 1 .. 3, got {tuple(cross_channel)!r}")
        else:
            raise TypeError(f"cross_channel must be False, True or a sequence of channel indices, got {cross_channel!r}")
        if attrs is None:
            raise ValueError("cross_channel predicts the channels of attributes: it needs attributes=")
        masks = []
        for f, a in enumerate(attrs):
            c = a.shape[1]
            if chans is None:
                masks.append((1 << (c - 1)) - 1)
                continue
            if chans and chans[-1] >= c:
                raise ValueError(f"frame {f}: cross_channel names channel {chans[-1]}, the frame has channels 0 .. {c - 1}")
            masks.append(sum(1 << (ch - 1) for ch in chans))
        return masks

    @staticmethod
    def _check_predictor(predictor, attrs, max_error, qstep, colour, scalable_to, target_bytes, target_frame_bytes):
        """predictor of compress -> "neighbours" (attribute blob versions 25 / 26), "bounded-neighbours" (28 / 31, which
        need max_error >= 1), or None"""
        if predictor is None:
            return None
        if not isinstance(predictor, str):
            raise TypeError(f"predictor must be None or 'neighbours' or 'bounded-neighbours', got {predictor!r}")
        if predictor not in ("neighbours", "bounded-neighbours"):
            raise ValueError(f"predictor must be None or 'neighbours' or 'bounded-neighbours', got {predictor!r}")
        if attrs is None:
            raise ValueError("predictor predicts the values of attributes: it needs attributes=")
        bounded = predictor == "bounded-neighbours"
        if bounded and not GeometryCodec._check_max_error(max_error, attrs):
            raise ValueError("predictor='bounded-neighbours' needs max_error >= 1 (attribute blob versions 28 and 31 bound every "
                             "value's error by it); predictor='neighbours' is the lossless kind")
        for name, given in (("max_error", bool(max_error) and not bounded),
                            ("qstep", not isinstance(qstep, (int, np.integer)) or bool(qstep)),
                            ("colour", colour is not None), ("scalable_to", scalable_to is not None),
                            ("target_bytes", target_bytes is not None), ("target_frame_bytes", target_frame_bytes is not None)):
            if given and bounded:
                raise ValueError(f"predictor='bounded-neighbours' with {name}: attribute blob versions 28 and 31 bound every "
                                 "value's error by max_error, they have no transform-coded form and no byte target")
            if given:
                raise ValueError(f"predictor='neighbours' with {name}: attribute blob versions 25 and 26 are lossless, the "
                                 "predictor from 3-D neighbours has no transform-coded form; its near-lossless form is "
                                 "predictor='bounded-neighbours' with max_error (attribute blob versions 28 and 31)")
        return predictor

    def compress(self, frames, attributes=None, lod=0, scalable=False, *, voxel=None, origin=(0.0, 0.0, 0.0),
                 invalid="raise", return_index=False, max_error=0, cross_channel=False, qstep=0, colour=None,
                 scalable_to=None, target_bytes=None, target_frame_bytes=None, predict=None, intra_period=None, reference=None,
                 history=None, predictor=None, attribute_scale=None, attribute_dtype=None):
        """frames: a sequence of int16 / int32 [n_f, 3] arrays -> a list of bytes, one version-2 blob per frame.
        Duplicate points are removed (as np.unique), out-of-range coordinates raise PccError (PCC_E_RANGE).
        lod = k > 0: the sender's side of a level of detail — blob f is the version-2 blob of the distinct cells
        points_f >> k (under bias 32768 >> k), which every decoder reads as those cell indices; the rows of a CELL
        merge as duplicate points do, in one merge over all input rows of the cell.
        attributes (optional): one uint8 / uint16 [n_f] or [n_f, c] array per frame (1 <= c <= 4) -> (blobs,
        attribute blobs): attribute blob f holds, losslessly, one row per decoded point of frame f (Morton order), the
        rows of duplicate points merged to their rounded mean per channel.  scalable=True: attribute blobs of version 2,
        whose coarser levels of detail are prefixes (attr_lod_info, decompress(..., lod=k)); the geometry blobs are the
        same, the default stays version 1.  With lod = k it codes the cells' means over the cells' keys.
        max_error = e > 0 (an integer; bool or non-integer: TypeError; negative, without attributes, or 2^(8 bytes per
        value - 1) and more for a frame's dtype: ValueError): near-lossless attribute blobs, version 4 (7 with
        scalable=True) — no decoded value is off by more than e from what max_error=0 returns for the same call, at
        every level of detail (attr_info reads e back from a blob).  The geometry blobs are the same; 0, the default, is
        the lossless coder and its bytes.
        cross_channel: False (the default, the bytes of before); True — in every frame each channel 1 .. c_f - 1 is coded
        against the channel before it, attribute blob versions 8 / 11 / 13 / 14 in place of 1 / 2 / 4 / 7 (include/pcc.h
        has the rule), a frame of one channel keeps its plain kind; or a sequence of distinct channel indices in 1 .. 3,
        those channels only — (1, 2) for RGB beside an unrelated fourth channel — where an index no frame f has raises
        ValueError naming f.  Anything else: TypeError; without attributes: ValueError.  The decoded values are exactly
        those of the same call without it, at every level of detail and under max_error; the geometry blobs are the same.
        For correlated channels (a camera's colour: about a fifth smaller); uncorrelated ones grow, the sender chooses.
        qstep = q > 0 (an integer; bool or non-integer: TypeError; negative, without attributes, or 2^(8 bytes per value -
        1) and more for a frame's dtype: ValueError naming the frame; with max_error, scalable=True or cross_channel:
        ValueError saying why): transform-coded attribute blobs, version 19 (include/pcc.h has the rule) — lossy, for
        rates below about a byte per point, where max_error's staircase is the wrong tool: on recorded camera colour
        q = 32 gives fewer bytes than max_error=16 at two thirds of its mean squared error.  No single value's error is
        bounded, and the step never falls below 2, so the kind has no lossless setting (q = 1 is its finest).  It
        combines with lod=k (the cells' means over the cells' keys), float32 / device frames, invalid="drop" and
        return_index; decompress reads it at lod 0 only.  The geometry blobs are the same; 0, the default, is the bytes
        of before (attr_info reads q back from a blob).
        qstep a tuple / list of integers: one step per channel, attribute blob version 21 (include/pcc.h has the rule) —
        version 19 with a step of its own for every channel, for RGB beside an unrelated fourth channel, or chroma coarser
        than luma.  A bool or non-integer entry: TypeError; an entry below 1, or 2^(8 bytes per value - 1) and more for
        a frame's dtype, or a length other than a frame's channel count: ValueError naming the frame.
        colour="ycocg": version 21 with the luma / chroma transform (YCoCg-R with the low bit of each chroma difference
        dropped; channels 0, 1, 2 are R, G, B, a fourth is untouched) in front of the lift: an integer qstep then serves
        every channel and drives Y, Co and Cg where it drove R, G and B.  On recorded camera colour q = 16 with it is
        shorter and closer than q = 32 without.  Without qstep: ValueError (the lossless and bounded kinds have
        cross_channel= for this); a frame of fewer than 3 channels: ValueError naming the frame; any other value:
        ValueError.  Both refuse max_error, scalable=True and cross_channel as qstep does, and combine with lod=k,
        float32 / device frames, invalid="drop" and return_index as it does.  An integer qstep without colour stays
        version 19, the bytes of before.
        scalable_to = K (with qstep; an integer in 1 .. 15 - lod; bool or non-integer: TypeError; out of range, without
        qstep, or with max_error, cross_channel or scalable=True: ValueError): attribute blob version 22 (include/pcc.h
        has the rule) — version 21 under weights that a decoder at a cut can form (K-cell counts above K, the level
        alone inside a K-cell), so that levels of detail 0 .. K are prefixes of the blob (attr_lod_info,
        decompress(..., lod=j)) at a few per cent more bytes than version 19 at equal error.  An integer qstep serves
        every channel; colour=, lod=k, float32 / device frames, invalid="drop" and return_index combine with it as with
        version 21.  None, the default, writes the bytes of before.
        target_bytes = B (with qstep; an integer >= 1 or a sequence of one per frame; bool or non-integer: TypeError;
        below 1, another length than the frames, without qstep, or with scalable_to: ValueError): a byte budget for the
        attribute blobs.  qstep is then the finest setting the sender accepts; every frame is coded at the first setting
        of the ladder rate_ladder(qstep, dtype) that the search of include/pcc.h finds with len(attr_blobs[f]) <= B
        (quarter-octave steps, all channels coarsened together), in one call: merge, colour transform and lift run once,
        the candidates are coded side by side.  The blob is byte for byte the one compress writes at those steps
        (version 19 or 21; attr_info(blob)["qstep"] says which it got); a frame that the coarsest setting does not bring
        under B gets that setting and is longer than B.  target_frame_bytes = B bounds len(blobs[f]) +
        len(attr_blobs[f]) the same way: the attributes get what the frame's geometry blob leaves.  The two exclude each
        other.  Both combine with colour, lod=k, float32 / device frames, invalid="drop" and return_index as qstep
        does.  rate_scratch_limit (an attribute of the codec, bytes; 0: the library's default of 1 GiB) bounds the scratch
        of the candidates; the bytes do not depend on it.  None, the default, writes the bytes of before.

        Frame types: numpy int16 / int32 as above, numpy float32, or torch tensors of those three dtypes on the host or
        on this codec's device; all frames of a call integer or all float32, all on the host or all on the device
        (ValueError naming the frame otherwise; a tensor on another device: ValueError; float64: TypeError).  Device
        frames are not staged through the host.
        Attribute types: numpy uint8 / uint16 as above (the staging and the bytes of before), or torch tensors of those
        two dtypes on this codec's device, read where they lie (pcc_attr_stage_frames; include/pcc.h has the rule): a
        view whose rows are contiguous, such as t[:, 4:7] of an interleaved tensor, goes in by its pitch, any other view
        is made contiguous first.  The attributes of a call are all on the host or all on the device (ValueError naming
        the frame; a tensor on another device: ValueError), whatever the place of the frames.  The caller's current
        stream is waited for before the first read, as it is for device frames.
        attribute_scale = s (a finite number, 0 < s <= 65535; bool or not a number: TypeError; out of range, without
        attributes, or beside integer attributes: ValueError): the attributes are float32 / float64, on the host or on
        the device, and every value becomes clip(rint(x * s), 0, peak) in its own precision, ties to even, on the device
        for both places, so both give the same blobs.  attribute_dtype: np.uint8 or np.uint16 (anything else:
        ValueError), what they become; the default is uint8 where s <= 255, else uint16.  A NaN or Inf value raises
        PccError (PCC_E_RANGE).  s is not written into a blob: decompress returns the integers and the caller carries s,
        as it carries voxel.  Float attributes without attribute_scale, and any other dtype (int32, float16): TypeError.
        voxel, origin: float32 frames are points in the caller's unit and need voxel > 0; the codec codes the lattice
        points q = rint((x - origin) / voxel), per coordinate in float32 (include/pcc.h has the rule; voxel and origin
        are narrowed to float32 once, and the blobs are those of compress([q])).  Neither is written into a blob.
        Integer frames refuse voxel (ValueError).
        invalid: "raise" — a non-finite coordinate, or a q outside [-32768, 32767], raises PccError (PCC_E_RANGE) that
        says which; "drop" — rows with a non-finite coordinate (beams without a return) are left out before coding,
        a frame of such rows alone gives the 24-byte empty blob; a finite coordinate off the grid still raises.  No
        effect on integer frames.
        return_index=True appends `index` to the result, (blobs, index) or (blobs, attr_blobs, index): index[f] is int32
        [n_f], index[f][i] the row of decompress(blobs)[f] that input row i became (duplicates share a row; with lod = k
        the row of the cell), -1 for a dropped row; numpy arrays for host frames, device tensors for device frames.
        predict="previous" (any other value but None: ValueError): inter-frame prediction — every frame but the intra
        ones is a blob of version 4 (include/pcc.h has the rule), coded against the frame in front of it in the call,
        about a fifth shorter for consecutive LiDAR sweeps; decompress needs the frames in front of it back to an intra
        frame (geometry_info says which blobs those are).  intra_period = G (an integer >= 1; bool or non-integer:
        TypeError; below 1, or without predict: ValueError): frames 0, G, 2 G, .. are intra (version 2, the bytes of
        before); None: frame 0 alone.  reference (without predict: ValueError): one frame of the same kind and place as
        `frames`, put through the same front end (voxel, invalid, duplicates, lod) as frame -1 of the call, so that
        frame 0 is predicted too — a streaming sender codes one frame per call against the last.  history = K (an
        integer in 1 .. 8; bool or non-integer: TypeError; out of range, or without predict: ValueError): a predicted
        frame is coded against the union of its window, the up to K frames in front of it, which reaches neither past an
        intra frame (that frame may be in it) nor past a frame without points; reference may then be a list or tuple of
        1 .. K frames, oldest first (more: ValueError).  None and 1 are the call of before.  A frame without
        points stays the 24-byte blob, and the frame behind it (or behind a reference without points) is intra.
        Attributes of every kind, lod=k (frame and reference are both the cells), float32 and device frames,
        return_index and the byte targets combine with it as before: they see the decoded Morton order alone.  The
        defaults write the bytes of before.
        predict="best": intra_period, reference and history mean what they mean under "previous", and every coded
        frame that is not a scheduled intra frame is written as the shortest of its candidates — its version-2 blob
        and, for W in 1 .. the window history=K gives it (None and 1: W = 1 alone), its version-4 blob against the
        union of the W frames in front of it; of equal lengths version 2, then the smaller W.  Every blob is byte for
        byte the one predict=None or predict="previous", history=W writes for the frame.  A version-2 blob written by
        choice cuts no window: the frames behind it may reach past it, and only the scheduled intra frames are
        random-access points.  It combines with everything "previous" combines with; target_frame_bytes reads the
        lengths after the choice.
        predictor="neighbours" (with attributes; another string: ValueError, another type: TypeError): lossless
        attribute blobs of version 25 (include/pcc.h has the rule) — version 2's layout and prefixes, every value
        predicted from up to three Morton-first points of the coarser cells around its point instead of from one, about
        a tenth smaller than versions 1 and 2 on colour; version 26, its cross-channel form, for the frames that
        cross_channel gives a mask.  The blobs are always cuttable (attr_lod_info, decompress(..., lod=k)): scalable=True
        or False beside it changes nothing.  It combines with lod=k, float32 / device frames, invalid="drop",
        return_index, predict= / history= (geometry only) and cross_channel; with max_error, qstep, colour, scalable_to,
        target_bytes or target_frame_bytes: ValueError saying why (the kind is lossless and has no transform-coded
        form).  None, the default, writes the bytes of before.
        predictor="bounded-neighbours" with max_error=e >= 1 (without it, or with e = 0: ValueError, "neighbours" is the
        lossless kind): attribute blobs of version 28, version 7's layout and prefixes with the same three candidates in
        a closed loop — every value is predicted from its candidates' decoded values, the error of the prediction is
        quantised with step 2 e + 1, and no decoded value is off by more than e; 11 to 25 % smaller than version 7 on
        colour at e = 1 .. 8.  Version 31 is its cross-channel form.  Always cuttable (scalable= changes nothing); a row
        at lod k is within e of the row predictor="neighbours" gives there.  It combines with what "neighbours" combines
        with; qstep, colour, scalable_to, target_bytes or target_frame_bytes beside it: ValueError naming the keyword.
        max_error's own checks (type, sign, the dtype's 2^(8 bpv - 1)) are unchanged."""
        lod = self._check_lod(lod)
        frames, is_float, on_device = self._check_frames(frames)
        intra_period, reference, history = self._check_predict(predict, intra_period, reference, is_float, on_device, len(frames),
                                                               history)
        self._check_invalid(invalid)
        voxel, origin = self._check_voxel(is_float, voxel, origin, "compress")
        scale, attr_dtype = self._check_attribute_scale(attribute_scale, attribute_dtype, attributes is not None)
        attrs = None if attributes is None else self._check_attributes(frames, attributes, self._device, scale, attr_dtype)
        nb = len(frames)
        neighbours = self._check_predictor(predictor, attrs, max_error, qstep, colour, scalable_to, target_bytes, target_frame_bytes)
        coding = self._attr_coding(attrs, nb, lod, scalable, max_error, cross_channel, qstep, colour, scalable_to, target_bytes,
                                   target_frame_bytes)
        if neighbours == "neighbours":
            coding = coding._replace(version=2, neighbours=True)
        elif neighbours:
            coding = coding._replace(version=2, neighbours_nl=True)
        if coding is not None and coding.targets is not None:
            coding = coding._replace(scratch_limit=int(self.rate_scratch_limit))

        def result(blobs, attr_blobs=None, index=None):
            out = (blobs,) if attrs is None else (blobs, attr_blobs)
            if return_index:
                out += (index,)
            return out[0] if len(out) == 1 else out
        if nb == 0:
            return result([], [], [])
        attrs_on_device = self._staged(attrs) and attrs[0].on_device
        caller = torch.cuda.current_stream(self.rt.device) if on_device or attrs_on_device else None      # inside `with rt` it is the codec's
        with self._lock, self.rt as rt:
            front = self._front(rt, frames, is_float, on_device, caller, "GeometryCodec.compress", lod, voxel, origin,
                                invalid == "drop")
            if front.n_keep == 0:
                return result(*self._nothing_coded(rt, front, attrs, coding, return_index, on_device, caller, scale))
            if predict is None:
                blobs = rt.octree_encode_frames(front.keys, nb, 3 * lod)
            else:
                blobs = self._encode_predicted(rt, front, nb, lod, intra_period, reference, is_float, on_device, caller, voxel,
                                               origin, invalid == "drop", history, predict == "best")
            attr_blobs = index = None
            if attrs is not None:
                if target_frame_bytes is not None:      # what the geometry blob leaves; nothing left: a target no blob meets, the coarsest steps
                    coding = coding._replace(targets=tuple(max(1, t - len(b)) for t, b in zip(coding.targets, blobs)))
                attr_blobs = self._encode_attributes(rt, attrs, blobs, front, 3 * lod, coding, caller, scale)
            if return_index:
                first_run = torch.empty(nb, dtype=torch.int64, pin_memory=True)
                np.cumsum([0] + [struct.unpack_from("<I", b, 4)[0] for b in blobs[:-1]], out=first_run.numpy())
                index = rt.rows_index(front.perm, front.n_keep, front.rows, front.n_unique, front.offsets.data_ptr(),
                                      rt.to_device(first_run), nb)
                index = self._split_index(index, front.sizes, on_device)
            return result(blobs, attr_blobs, index)

    def _check_predict(self, predict, intra_period, reference, is_float, on_device, nb, history=None):
        """predict, intra_period, reference and history of compress -> (the period the library takes: 0 = frame 0
        alone; the references as _check_frames returns frames, oldest first, or None; the window K)"""
        if predict is not None and not (isinstance(predict, str) and predict in ("previous", "best")):
            raise ValueError(f"predict must be None, 'previous' or 'best', got {predict!r}")
        if intra_period is not None:
            if isinstance(intra_period, bool) or not isinstance(intra_period, (int, np.integer)):
                raise TypeError(f"intra_period must be an integer >= 1, got {intra_period!r}")
            if intra_period < 1:
                raise ValueError(f"intra_period must be an integer >= 1, got {intra_period}")
            if predict is None:
                raise ValueError("intra_period is the distance of the intra frames under prediction: it needs predict='previous'")
        if history is not None:
            if isinstance(history, bool) or not isinstance(history, (int, np.integer)):
                raise TypeError(f"history must be an integer in 1 .. {MAX_HISTORY}, got {history!r}")
            if not 1 <= history <= MAX_HISTORY:
                raise ValueError(f"history must be an integer in 1 .. {MAX_HISTORY}, got {history}")
            if predict is None:
                raise ValueError("history is how many frames a predicted frame is coded against: it needs predict='previous'")
        history = int(history or 1)
        if reference is None:
            return int(intra_period or 0), None, history
        if predict is None:
            raise ValueError("reference is what frame 0 is predicted from: it needs predict='previous'")
        several = isinstance(reference, (list, tuple))
        if several and not 1 <= len(reference) <= history:
            raise ValueError(f"reference: {len(reference)} frames, history={history} takes 1 .. {history} (oldest first)")
        try:
            refs, ref_float, ref_device = self._check_frames(list(reference) if several else [reference])
        except (TypeError, ValueError) as e:
            raise type(e)("reference: " + (str(e) if several else str(e).replace("frame 0: ", ""))) from None
        if nb and (ref_float != is_float or ref_device != on_device):
            raise ValueError("reference: one frame of the same kind (integer or float32) and place (host or device) as the frames")
        return int(intra_period or 0), refs, history

    def _encode_predicted(self, rt, front, nb, lod, intra_period, reference, is_float, on_device, caller, voxel, origin, drop,
                          history=1, best=False):
        """the geometry blobs of a call under predict='previous' or, best, 'best': the call's distinct keys, behind the
        references' as the first frames of the library's call where there are any.  history 1 is the call of before."""
        m = 0 if reference is None else len(reference)
        if m:
            ref = self._front(rt, reference, is_float, on_device, caller, "GeometryCodec.compress (reference)", lod, voxel,
                              origin, drop)
            if ref.n_keep:      # (references without points predict nothing: frame 0 is intra)
                keys = torch.cat([ref.keys, front.keys + (m << 48)])
                if best:
                    return rt.octree_encode_frames_inter_best(keys, nb + m, 3 * lod, intra_period, m, history)
                if history == 1:
                    return rt.octree_encode_frames_inter(keys, nb + 1, 3 * lod, intra_period, ref_first=True)
                return rt.octree_encode_frames_inter_hist(keys, nb + m, 3 * lod, intra_period, m, history)
        if best:
            return rt.octree_encode_frames_inter_best(front.keys, nb, 3 * lod, intra_period, 0, history)
        if history == 1:
            return rt.octree_encode_frames_inter(front.keys, nb, 3 * lod, intra_period)
        return rt.octree_encode_frames_inter_hist(front.keys, nb, 3 * lod, intra_period, 0, history)

    @staticmethod
    def reference_frames(blob):
        """W, the number of decoded frames in front of its own that a version-4 blob's reference is the union of (byte
        3 of its head + 1; compress(..., history=K) writes 1 .. K); 0 for a version-2 blob.  Host only: the head alone."""
        blob = bytes(blob[:4])
        if len(blob) < 4 or blob[0] != ord("O") or blob[1] not in (2, 4):
            raise ValueError("not an octree blob of version 2 or 4")
        return blob[3] + 1 if blob[1] == 4 else 0

    @staticmethod
    def geometry_info(blob):
        """what the head of a geometry blob of version 2 or 4 says: {"version", "points", "predicted",
        "reference_points"} — predicted False marks a random-access point of a sequence, a predicted blob decodes
        only behind the frame it was coded against, whose point count is reference_points.  Under
        compress(..., predict="best") that holds for the scheduled intra frames alone: a version-2 blob chosen for its
        length decodes alone too, but a frame behind it may reach past it.  Host only; the blob whole, or for version 4
        exactly a prefix that lod_info names."""
        return Runtime.octree_inter_info(bytes(blob))

    @staticmethod
    def _attr_coding(attrs, nb, lod, scalable, max_error, cross_channel, qstep, colour, scalable_to, target_bytes, target_frame_bytes):
        """the attribute keywords of compress -> the AttrCoding its attribute blobs are written under, None without
        attributes: the checkers run, and raise, with and without them.  A target is the keyword's: what a frame's
        geometry blob takes of target_frame_bytes comes off where the blobs are known, and the codec's scratch limit is
        compress's to add."""
        G = GeometryCodec
        max_error = G._check_max_error(max_error, attrs)
        cross = G._check_cross(cross_channel, attrs)
        qstep, steps, colour = G._check_colour(qstep, colour, attrs, max_error, scalable, cross)
        steps, scalable_to = G._check_scalable_to(scalable_to, lod, qstep, steps, attrs, max_error, scalable, cross)
        targets, _ = G._check_rate(target_bytes, target_frame_bytes, nb, qstep, scalable_to)
        if attrs is None:
            return None
        # versions 21 and 22: a step per channel; else the one integer step of version 19, or 0
        return AttrCoding.of(2 if scalable else 1, max_error, cross, qstep if steps is None else steps, colour, scalable_to, targets)

    def _front(self, rt, frames, is_float, on_device, caller, where, lod=0, voxel=None, origin=None, drop=False):
        """the frames of a call -> _Front: stage, keys, sorted / distinct.  Called under `with self._lock, self.rt`;
        `caller` is the stream that was current before that block (device frames), `where` the origin an error names."""
        sizes = [int(a.shape[0]) for a in frames]
        n = int(sum(sizes))
        if n == 0:
            return _Front(len(frames), sizes, 0, 0)
        offsets, xyz, dtype = self._stage(rt, frames, sizes, is_float, on_device, caller)
        keys, n_keep, flag = self._keys(rt, offsets, xyz, dtype, n, len(frames), where, voxel, origin, drop)
        return self._distinct(rt, _Front(len(frames), sizes, n, n_keep, offsets), keys, flag, lod, where)

    @staticmethod
    def _stage(rt, frames, sizes, is_float, on_device, caller):
        """one upload, the rows as they come (6 or 12 B per point) at the next 16-byte boundary behind the int64 frame
        offsets; the frame index and the widening to keys happen on the device.  Device frames send the offsets alone
        and are concatenated once on the device.  -> (the upload, the rows on the device, their numpy dtype)"""
        if is_float:
            dtype = np.float32
        else:
            dtype = np.int16 if all(a.element_size() == 2 if on_device else a.dtype == np.int16 for a in frames) else np.int32
        offs_b = 8 * (len(frames) + 1)
        rows_at = (offs_b + 15) // 16 * 16
        host_rows = 0 if on_device else 3 * sum(sizes) * np.dtype(dtype).itemsize
        host = torch.empty(rows_at + host_rows, dtype=torch.uint8, pin_memory=True)
        h = host.numpy()
        np.cumsum([0] + sizes, out=h[:offs_b].view(np.int64))
        if not on_device:
            np.concatenate(frames, axis=0, out=h[rows_at:].view(dtype).reshape(-1, 3))
        dev = rt.to_device(host)
        if not on_device:
            return dev, dev[rows_at:], dtype
        rt.stream.wait_stream(caller)      # behind whatever the caller's stream still does to the frames
        tdtype = {np.float32: torch.float32, np.int16: torch.int16, np.int32: torch.int32}[dtype]
        return dev, torch.cat([a.detach().to(tdtype) for a in frames], 0).contiguous(), dtype

    @staticmethod
    def _keys(rt, offsets, xyz, dtype, n, nb, where, voxel, origin, drop):
        """-> (the call's n Morton keys, frame index above bit 48; n_keep; the integer kernel's range flag, not read
        yet, or None).  float32 reads its status here, behind one synchronisation in place of the flag's."""
        if dtype == np.float32:
            keys, status = rt.morton_keys_frames_f32(xyz.data_ptr(), n, offsets.data_ptr(), nb, voxel, origin, drop)
            bits, dropped = status.tolist()
            if bits & 2:
                raise PccError(PCC_E_RANGE, where, "non-finite coordinate (NaN or Inf) in a frame; "
                               "invalid='drop' leaves such rows out")
            if bits & 1:
                raise PccError(PCC_E_RANGE, where, "coordinate outside [-32768, 32767] after "
                               "rint((x - origin) / voxel): a finite point off the grid")
            return keys, n - dropped, None
        keys = rt.empty((n,), torch.int64)
        flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
        check(rt.lib.pcc_morton_keys_frames(rt.ctx, C.c_void_p(xyz.data_ptr()), np.dtype(dtype).itemsize, n,
                                            C.c_void_p(offsets.data_ptr()), nb, _ptr(keys), _ptr(flag)),
              "pcc_morton_keys_frames")
        return keys, n, flag

    @staticmethod
    def _distinct(rt, front, keys, flag, lod, where):
        """sort, cut to the kept rows, lod mask, duplicates (np.unique) -> `front` filled in"""
        perm = rt.sort_pairs(keys)
        n_keep = front.n_keep
        if n_keep < front.n:      # the dropped rows' keys sorted behind every frame's: nothing below sees them
            keys = keys[:n_keep]
        if n_keep == 0:
            return front
        if lod:      # a cell's keys differ in their low 3 lod bits only (the batch index above bit 48 stays)
            keys.bitwise_and_(-(1 << (3 * lod)))
        rows = rt.empty((n_keep,), torch.int32)      # the first row of every run of equal keys
        n_u = C.c_int64(0)
        check(rt.lib.pcc_unique_rows(rt.ctx, _ptr(rt.keys_to_coords(keys)), n_keep, _ptr(rows), C.byref(n_u)),
              "pcc_unique_rows")
        if flag is not None and int(flag.item()) != 0:      # read behind the synchronisation of pcc_unique_rows
            raise PccError(PCC_E_RANGE, where, "coordinate outside [-32768, 32767]")
        distinct = keys if n_u.value == n_keep else rt.gather_rows(keys, rows[:n_u.value])
        return front._replace(perm=perm, sorted_keys=keys, rows=rows, n_unique=n_u.value, keys=distinct)

    def _nothing_coded(self, rt, front, attrs, coding, return_index, on_device, caller=None, scale=None):
        """(blobs, attribute blobs, index) of a call none of whose rows is coded: the empty blobs, the attribute blobs
        of frames without points (whatever the targets), and -1 for every input row"""
        blobs = rt.octree_encode_frames(rt.empty((0,), torch.int64), front.nb)
        attr_blobs = None if attrs is None else self._encode_attributes(rt, attrs, blobs, front, 0, coding._replace(targets=None),
                                                                                 caller, scale)
        if not return_index:
            return blobs, attr_blobs, None
        index = torch.full((front.n,), -1, dtype=torch.int32, device=rt.device)
        return blobs, attr_blobs, self._split_index(index, front.sizes, on_device)

    def _split_index(self, index, sizes, on_device):
        """the call's index [n] on the device -> one int32 [n_f] per frame: views of it (device frames), or of one
        copy of it on the host"""
        if on_device:
            self.rt.sync()      # the caller's stream may read it at once
        else:
            index = index.cpu().numpy()
        return _split(index, sizes)

    @staticmethod
    def _encode_attributes(rt, attrs, blobs, front, key_shift, coding, caller=None, scale=None):
        # the values as they come, frame by frame at 16-byte offsets, in one upload; the merge into Morton order
        # happens on the device from the sort's permutation and the runs of equal keys
        status = None
        if GeometryCodec._staged(attrs):      # device tensors and float values: the same layout, written by one kernel
            values, offs, status = GeometryCodec._stage_attributes(rt, attrs, caller, scale)
            if scale is None:
                status = None      # integers as they are: nothing to report
        else:
            offs, at = [], 0
            for a in attrs:
                offs.append(at)
                at += (a.nbytes + 15) // 16 * 16
            host = torch.empty(max(at, 16), dtype=torch.uint8, pin_memory=True)
            h = host.numpy()
            for o, a in zip(offs, attrs):
                h[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
            values = rt.to_device(host) if at else None
        formats = [a.dtype.itemsize | (a.shape[1] << 8) for a in attrs]
        points = [struct.unpack_from("<I", b, 4)[0] for b in blobs]
        n_kept = front.n_keep if front.n_keep < front.n else None      # None: no row was dropped
        call = (values, offs, formats, _ends(front.sizes), points, front.perm, front.rows, front.n_unique, front.keys, key_shift, n_kept)
        if coding.targets is None:
            attr_blobs = rt._attr_encode(coding, *call)[0]
        else:
            # a byte target: the steps from qstep upwards that the search chooses, frame by frame, through the public binding
            attr_blobs = rt.attr_encode_frames_rate(*call, coding.qstep, coding.colour, list(coding.targets), coding.scratch_limit)[0]
        if status is not None:      # behind the encode's own synchronisation
            GeometryCodec._check_stage_status(status, "GeometryCodec.compress")
        return attr_blobs

    def decompress(self, blobs, attr_blobs=None, output="numpy", lod=0, *, voxel=None, origin=(0.0, 0.0, 0.0), reference=None,
                   reference_lod=None):
        """version-2 blobs -> a list of int32 [n_f, 3] point sets in Morton order: numpy arrays (output="numpy") or
        device tensors (output="device", on this codec's device).  With attr_blobs (compress(..., attributes=...)):
        (point sets, attributes), attributes[f] an [n_f, c] array in its original dtype, row i belonging to point i; an
        attribute blob decodes only with the geometry blob of its own frame (another point count raises PccError).
        lod = k > 0: blobs or prefixes of them (lod_info) -> the distinct cell indices points >> k of every frame, int32
        [cells, 3] in Morton order (corner of a cell c << k, centre (c << k) + ((1 << k) >> 1)); with attr_blobs of
        version 2 (compress(..., scalable=True)), or prefixes of them (attr_lod_info): attributes[f] is [cells, c], row j
        the value of the Morton-first point of cell j.  The kind of every attribute blob (lossless 1 / 2, near-lossless
        4 / 7 of compress(..., max_error=e), their cross-channel forms 8 / 11 / 13 / 14 of compress(...,
        cross_channel=...), transform-coded 19 of compress(..., qstep=q) and 21 of compress(..., qstep=(..)) or
        colour="ycocg") is read from the blob; version 7 behaves as version 2 and its prefixes do, every value within e,
        and a cross-channel kind returns what its plain kind returns.  Version 22 (compress(..., qstep=q,
        scalable_to=K)) decodes at lod 0 .. K, from whole blobs or attr_lod_info's prefixes: row j is the mean of cell j
        under the kind's weights; lod > K raises ValueError naming the frame and K.  Versions 25 / 26 (compress(...,
        predictor="neighbours")) decode at every lod as versions 2 / 11 do, versions 28 / 31 (predictor=
        "bounded-neighbours") as 7 / 14 do, every value within their e.  The fifteen kinds may be mixed at
        lod 0; an attribute blob of version 1, 4, 8, 13, 19 or 21 at lod > 0 raises ValueError naming the frame.
        voxel (with origin): the point sets come back as float32 [n_f, 3] in the caller's unit instead of int32,
        x = origin + t * voxel, one float32 multiplication and then one addition on the device (include/pcc.h has the
        rule): t the lattice index at lod 0 and, at lod k, the centre of the cell's lattice points
        (c << k) + (2^k - 1) / 2 — a half-integer, not the integer centre above, which stays the centre in lattice
        units.  The blobs do not hold voxel or origin: pass what compress was given.  Attributes are unchanged.
        Blobs of version 4 (compress(..., predict="previous")) may stand among the blobs: each is decoded against the
        frame decoded before it in the call, blob 0 against `reference` — an int16 / int32 [n, 3] lattice frame, numpy or
        on this codec's device, in any row order and with duplicates: the decoded frame before it; or, for blobs of
        compress(..., history=K), a list or tuple of the up to 8 frames decoded before it, oldest first — a blob says
        itself (reference_frames) how many of the frames in front of it its reference is the union of.  Without the
        reference, or with another one than the sender's, PccError names the frame.
        Version 4 at lod = k > 0: blobs or their lod_info prefixes, chains, intra_period mixes and history windows as at
        lod 0, to the same cells as version 2's; scalable attribute blobs decode beside them.  A predicted frame is then
        decoded against the CELLS of the frames in front of it, so `reference` needs reference_lod to say what its rows
        are: reference_lod=k, the cells that the decompress(..., lod=k) before returned (a receiver that never held
        full resolution), or reference_lod=0, lattice points, whose cells the codec forms on the device.  Without it
        ValueError names the first version-4 frame; any other value is a ValueError.  A cut cannot verify the
        reference (the blob's count and sum describe full-resolution points): a wrong one is a PccError where the
        stream's counts do not add up and otherwise rows of wrong cells.  A call without a version-4 blob is the call
        of before."""
        if isinstance(attr_blobs, str):      # decompress(blobs, "device"), as before attributes
            attr_blobs, output = None, attr_blobs
        self._check_output(output)
        lod = self._check_lod(lod)
        if voxel is not None:
            voxel, origin = self._check_grid(voxel, origin, "decompress")
        blobs = [bytes(b) for b in blobs]
        if len(blobs) > MAX_FRAMES:
            raise ValueError(f"{len(blobs)} blobs in one call, at most {MAX_FRAMES}")
        ref_device = False
        several = isinstance(reference, (list, tuple))
        if several and not 1 <= len(reference) <= MAX_HISTORY:
            raise ValueError(f"reference: {len(reference)} frames, a blob's reference is the union of 1 .. {MAX_HISTORY} (oldest first)")
        if reference is not None:
            try:
                reference, ref_float, ref_device = self._check_frames(list(reference) if several else [reference])
            except (TypeError, ValueError) as e:
                raise type(e)("reference: " + (str(e) if several else str(e).replace("frame 0: ", ""))) from None
            if not several:
                (reference,) = reference
            if ref_float:
                raise TypeError("reference: expected the int16 / int32 lattice frame that was decoded before blob 0, got float32")
        predicted = [f for f, b in enumerate(blobs) if len(b) > 1 and b[1] == 4]
        if reference_lod is not None:
            if (not isinstance(reference_lod, (int, np.integer)) or isinstance(reference_lod, bool) or reference is None
                    or int(reference_lod) not in (0, lod)):
                raise ValueError(f"reference_lod says what the rows of reference= are at lod {lod}: {lod} (the cells of a "
                                 f"decompress at that lod) or 0 (lattice points), got {reference_lod!r}"
                                 + ("" if reference is not None else " without a reference"))
            reference_lod = int(reference_lod)
        elif predicted and lod and reference is not None:
            raise ValueError(f"frame {predicted[0]}: blob version 4 (a predicted frame) at lod {lod}: the rows of reference= may be "
                             f"cells or lattice points; say which with reference_lod={lod} (the cells that "
                             f"decompress(..., lod={lod}) returned) or reference_lod=0 (lod 0 lattice points)")
        if attr_blobs is not None:
            attr_blobs = [bytes(b) for b in attr_blobs]
            if len(attr_blobs) != len(blobs):
                raise ValueError(f"{len(attr_blobs)} attribute blobs for {len(blobs)} geometry blobs")
            kind = [b[1] if len(b) > 1 else 0 for b in attr_blobs]      # runs of one kind are decoded in one call
            v1 = [k in ATTR_RUN_KINDS for k in kind]
            if lod and any(k in ATTR_TRANSFORM_KINDS for k in kind):
                f = min(kind.index(k) for k in ATTR_TRANSFORM_KINDS if k in kind)
                raise ValueError(f"frame {f}: attributes of blob version {kind[f]} cannot be decoded at lod > 0: the weights of "
                                 "its transform are the point counts under every node, which a decoder at a cut does not "
                                 "have; store version 2, 7, 11 or 14 (compress(..., scalable=True)) or ship coarse "
                                 "attributes with compress(frames, attributes=..., lod=k, qstep=q)")
            for f, b in enumerate(attr_blobs):      # version 22: up to the K its sender chose
                if lod and kind[f] == ATTR_SCALABLE_TRANSFORM_KIND and len(b) >= 8 and struct.unpack_from("<I", b, 4)[0]:
                    to = Runtime.attr_info(b)["scalable_to"]
                    if lod > to:
                        raise ValueError(f"frame {f}: attributes of blob version 22 with scalable_to = {to} cannot be decoded at "
                                         f"lod {lod}: its sender chose {to} as the deepest cut")
            if lod and any(v1):
                raise ValueError(f"frame {v1.index(True)}: attributes of blob version {kind[v1.index(True)]} cannot be decoded at lod > 0: it "
                                 "is one predictive stream in full-resolution Morton order, so neither its bytes nor "
                                 "its decoding can be cut; store version 2, 7, 11 or 14 (compress(..., scalable=True)) or ship "
                                 "coarse attributes with compress(frames, attributes=..., lod=k)")
        caller = torch.cuda.current_stream(self.rt.device) if (predicted and ref_device) else None
        with self._lock, self.rt as rt:
            if predicted and lod:      # at a cut: the references are cells, given or formed here from lattice points
                refs = []
                if reference is not None:
                    frames_in = list(reference) if several else [reference]
                    front = self._front(rt, frames_in, False, ref_device, caller, "GeometryCodec.decompress (reference)",
                                        lod if reference_lod == 0 else 0)
                    refs = [torch.empty((0, 3), dtype=torch.int32, device=rt.device)] * len(frames_in)
                    if front.n_keep:      # distinct and in Morton order, split by the frame index of the keys
                        coords = rt.keys_to_coords(front.keys)
                        ends = torch.searchsorted(coords[:, 0].contiguous(), torch.arange(len(frames_in) + 1, device=rt.device,
                                                                                          dtype=coords.dtype)).tolist()
                        shift = lod if reference_lod == 0 else 0      # a masked key's coordinates are the cell's corner
                        refs = [(coords[a:b, 1:] >> shift).contiguous() for a, b in zip(ends[:-1], ends[1:])]
                    if not several and not refs[0].shape[0]:
                        refs = []
                decode = lambda blobs, device, lod, whole=False: rt.octree_decode_frames_refs_lod(blobs, refs, lod, device=device, whole=whole)   # noqa: E731
            elif predicted:      # the new entry point, and the reference as a decode returns it: distinct, Morton order
                ref = None
                if several:      # each as a decode returns it; one front end for all, split by the frame index of the keys
                    front = self._front(rt, reference, False, ref_device, caller, "GeometryCodec.decompress (reference)")
                    ref = [torch.empty((0, 3), dtype=torch.int32, device=rt.device)] * len(reference)
                    if front.n_keep:
                        coords = rt.keys_to_coords(front.keys)
                        ends = torch.searchsorted(coords[:, 0].contiguous(), torch.arange(len(reference) + 1, device=rt.device,
                                                                                          dtype=coords.dtype)).tolist()
                        ref = [coords[a:b, 1:].contiguous() for a, b in zip(ends[:-1], ends[1:])]
                    decode = lambda blobs, device, lod, whole=False: rt.octree_decode_frames_refs(blobs, ref, device=device, whole=whole)   # noqa: E731
                else:
                    if reference is not None and reference.shape[0]:
                        front = self._front(rt, [reference], False, ref_device, caller, "GeometryCodec.decompress (reference)")
                        ref = rt.keys_to_coords(front.keys)[:, 1:].contiguous()
                    decode = lambda blobs, device, lod, whole=False: rt.octree_decode_frames_ref(blobs, ref, device=device, whole=whole)   # noqa: E731
            else:
                decode = lambda blobs, device, lod, whole=False: rt.octree_decode_frames(blobs, device=device, lod=lod, whole=whole)   # noqa: E731
            # version 2 reads the cells where the geometry decode left them: on the device
            one_call = attr_blobs is not None and all(v1) and len(set(kind)) == 1
            on_device = attr_blobs is not None and not one_call
            if voxel is not None:      # the points in the caller's unit, dequantised where the decode left them
                cells, whole = decode(blobs, device=True, lod=lod, whole=True)
                frames = self._metric_frames(rt, cells, whole, lod, voxel, origin, output)
            else:
                frames = decode(blobs, device=(output == "device" or on_device), lod=lod)
                cells = frames
            if attr_blobs is None:
                return frames
            if one_call:
                return frames, rt.attr_decode_frames(attr_blobs, points=[f.shape[0] for f in frames],
                                                     device=(output == "device"))
            if output == "numpy" and voxel is None:      # one copy of the call's cells to the host, split as the device tensor is
                frames = _split(torch.cat(cells).cpu().numpy(), [c.shape[0] for c in cells])
            attrs = [None] * len(blobs)
            f = 0
            while f < len(blobs):      # runs of frames of one version, each in one call
                g = f
                while g < len(blobs) and kind[g] == kind[f]:
                    g += 1
                if v1[f]:
                    call = lambda: rt.attr_decode_frames(attr_blobs[f:g], points=[c.shape[0] for c in cells[f:g]],
                                                         device=(output == "device"))
                else:
                    call = lambda: rt.attr_decode_frames(attr_blobs[f:g], device=(output == "device"), lod=lod,
                                                         cells=cells[f:g])
                attrs[f:g] = self._named(f, call)
                f = g
            return frames, attrs

    @staticmethod
    def _metric_frames(rt, cells, whole, lod, voxel, origin, output):
        """the decoded int32 cells of a call (views of the device tensor `whole`) as float32 points: views of one device
        tensor, or of one host copy of it (12 B per point, as the int32 result's)"""
        if whole is None:
            return []
        return _frames_out(rt, rt.points_to_metric(whole, lod, voxel, origin), [int(c.shape[0]) for c in cells], output == "numpy")

    @staticmethod
    def _sorted_values(rt, attrs, perm, dtype, channels):
        """the attribute rows of a call in the order of its sorted keys, as one [n, channels] device tensor of `dtype`:
        every frame widened to the call's common format (absent channels 0 on both sides, so their differences are 0),
        one upload, and the sort's permutation applied on the device"""
        n = int(sum(a.shape[0] for a in attrs))
        host = torch.zeros(max(n, 1) * channels * np.dtype(dtype).itemsize, dtype=torch.uint8, pin_memory=True)
        h = host.numpy()[:n * channels * np.dtype(dtype).itemsize].view(dtype).reshape(n, channels)
        at = 0
        for a in attrs:
            h[at:at + a.shape[0], :a.shape[1]] = a
            at += a.shape[0]
        dev = rt.to_device(host)[:h.nbytes].view(torch.uint8 if dtype == np.uint8 else torch.uint16).reshape(n, channels)
        return rt.gather_rows(dev, perm)

    @staticmethod
    def _sorted_any(rt, attrs, perm, dtype, channels, caller, scale, statuses):
        """_sorted_values for host integer attributes; device tensors and float values in one pass of
        pcc_attr_stage_frames instead, whose status word joins `statuses` for the caller to read behind its next
        synchronisation"""
        if not GeometryCodec._staged(attrs):
            return GeometryCodec._sorted_values(rt, attrs, perm, dtype, channels)
        values, _, status = GeometryCodec._stage_attributes(rt, attrs, caller, scale, channels, perm, dtype)
        statuses.append(status)
        return values

    @staticmethod
    def _check_k(k, name):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 3 <= k <= 32:
            raise ValueError(f"{name} must be an integer in 3 .. 32, got {k!r}")
        return int(k)

    @staticmethod
    def _frame_counts(keys, nb):
        """the distinct points of every frame of a call, from the frame index of its distinct keys"""
        return np.bincount(((keys >> 48) & 0xFFFF).to(torch.int32).cpu().numpy(), minlength=nb)

    @staticmethod
    def _refuse_few(front, where):
        """ValueError naming the first frame with 1 or 2 distinct points: three points and more span a plane"""
        for f, u in enumerate(GeometryCodec._frame_counts(front.keys, front.nb)):
            if 0 < u < 3:
                raise ValueError(f"frame {f}: {int(u)} distinct points in {where}: a normal needs at least 3")

    def normals(self, frames, k=16, viewpoint=None, output="numpy"):
        """Surface normals of lattice frames, estimated on the device (pcc_knn_frames; include/pcc.h has the rule) -> one
        float32 [n_f, 3] per frame, row i the unit normal of input row i: the eigenvector of the smallest eigenvalue of
        the scatter matrix of the point's k nearest neighbours among the frame's distinct points (the point itself
        included; exact, ties to the Morton-first point).  Duplicate rows share their point's normal.
        frames: as distortion takes them, int16 / int32, numpy or torch, all on the host or all on this codec's device;
        float32 frames raise TypeError: pass lattice points.  k: an integer in 3 .. 32 (ValueError).  viewpoint: three
        integers in lattice units (the sensor): every normal is flipped to n . (viewpoint - p) >= 0; None leaves the sign
        unspecified.  output: "numpy" arrays, or "device": views of one tensor on this codec's device.  An empty frame
        gives [0, 3]; a frame with 1 or 2 distinct points raises ValueError naming the frame."""
        k = self._check_k(k, "k")
        if viewpoint is not None:
            try:
                vp = [v for v in viewpoint]
            except TypeError:
                vp = []
            if len(vp) != 3 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and abs(int(v)) < 1 << 30
                                       for v in vp):
                raise ValueError(f"viewpoint must be three integers in lattice units, got {viewpoint!r}")
            viewpoint = [int(v) for v in vp]
        self._check_output(output)
        frames, is_float, on_device = self._check_frames(frames)
        if is_float:
            raise TypeError("normals: float32 frames: pass lattice points (int16 / int32) — the input of compress, or "
                            "what decompress returns without voxel=")
        nb = len(frames)
        if nb == 0:
            return []
        sizes = [int(a.shape[0]) for a in frames]
        if sum(sizes) == 0:
            none = torch.empty((0, 3), dtype=torch.float32, device=self.rt.device) if output == "device" else \
                np.zeros((0, 3), np.float32)
            return [none[:0] for _ in sizes]
        caller = torch.cuda.current_stream(self.rt.device) if on_device else None
        with self._lock, self.rt as rt:
            front = self._front(rt, frames, False, on_device, caller, "GeometryCodec.normals")
            self._refuse_few(front, "frames")
            distinct = rt.knn_frames(front.keys, nb, k, viewpoint=viewpoint)[3]
            return _frames_out(rt, rt.gather_rows(distinct, self._input_rows(rt, front)), sizes, output == "numpy")

    @staticmethod
    def _check_filter(method, k, std_ratio, min_neighbours, radius2):
        """the rule's keywords of filter -> ("statistical", k, R = rint(256 std_ratio)) or ("radius", m, radius2)"""
        if not (isinstance(method, str) and method in ("statistical", "radius")):
            raise ValueError(f"method must be 'statistical' or 'radius', got {method!r}")
        if method == "statistical":
            for name, v in (("min_neighbours", min_neighbours), ("radius2", radius2)):
                if v is not None:
                    raise ValueError(f"{name} is a keyword of method='radius', not of method='statistical'")
            k = GeometryCodec._check_k(16 if k is None else k, "k")
            std_ratio = 2.0 if std_ratio is None else std_ratio
            if isinstance(std_ratio, bool) or not isinstance(std_ratio, (int, float, np.integer, np.floating)):
                raise TypeError(f"std_ratio must be a number in 0 .. 255, got {std_ratio!r}")
            if not (np.isfinite(std_ratio) and 0 <= std_ratio <= 255):
                raise ValueError(f"std_ratio must be a number in 0 .. 255, got {std_ratio!r}")
            return method, k, Runtime.outlier_ratio(std_ratio)
        for name, v in (("k", k), ("std_ratio", std_ratio)):
            if v is not None:
                raise ValueError(f"{name} is a keyword of method='statistical', not of method='radius'")
        m = 4 if min_neighbours is None else min_neighbours
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
            raise TypeError(f"min_neighbours must be an integer in 1 .. 31, got {m!r}")
        if not 1 <= m <= 31:
            raise ValueError(f"min_neighbours must be an integer in 1 .. 31, got {m!r}")
        if radius2 is None:
            raise ValueError("method='radius' needs radius2=, the squared radius in lattice units")
        if isinstance(radius2, bool) or not isinstance(radius2, (int, np.integer)):
            raise TypeError(f"radius2 must be a non-negative integer (squared lattice units), got {radius2!r}")
        if radius2 < 0:
            raise ValueError(f"radius2 must be a non-negative integer (squared lattice units), got {radius2!r}")
        return method, int(m), int(radius2)

    def filter(self, frames, attributes=None, method="statistical", k=None, std_ratio=None, min_neighbours=None, radius2=None,
               return_mask=False, return_report=False, output="numpy", *, voxel=None, origin=(0.0, 0.0, 0.0), invalid="raise"):
        """Outlier removal in front of compress, on the device (include/pcc.h has both rules): the rows of every frame
        that are surface, in input order, as the caller gave them (dtype and values untouched) -> `kept`, one array per
        frame; (kept, attrs) with attributes; then `mask` (return_mask) and `report` (return_report) behind them.
        The verdicts are formed per frame over the frame's distinct lattice points by exact k nearest neighbours;
        duplicate rows share their point's verdict.
        method="statistical" (Open3D's remove_statistical_outlier): k, an integer in 3 .. 32 (default 16), the point
        itself included; std_ratio, a number in 0 .. 255 (default 2.0), taken as R / 256 with R = rint(256 std_ratio).  A
        point's score is the sum of floor(16 sqrt(d2)) over its neighbours, and a point stays iff its score is at most
        mean + std_ratio * (sample standard deviation) of its frame's scores, decided exactly in integers.
        method="radius" (remove_radius_outlier): a point stays iff at least min_neighbours (1 .. 31, default 4) OTHER
        points of its frame lie within radius2, a non-negative integer in squared lattice units.
        A keyword of the other method, an unknown method, a value out of range: ValueError; a bool or a value of the
        wrong type: TypeError (k: ValueError, as normals raises).
        frames: int16 / int32 lattice frames, or float32 frames with voxel= / origin= / invalid= exactly as compress
        quantises them (the verdict is formed on the lattice, the rows returned are the caller's floats; a row dropped
        under invalid="drop" is not kept); numpy or torch, all on the host or all on this codec's device.
        attributes: one array per frame as compress takes them (uint8 / uint16 / float32 / float64, [n] or [n, c] with
        c <= 4, host or device, views with a pitch): the kept rows come back as given, nothing is quantised or merged.
        return_mask: bool [n_f] per frame, row i the verdict of input row i.  return_report: per frame a dict of Python
        ints, "points" (distinct), "kept" (distinct kept), "rows_kept", and under "statistical" also "k_eff", "S1",
        "S2", "threshold".  output: "numpy" arrays, or "device": tensors on this codec's device.
        An empty frame comes back empty; a frame of one point is kept whole under "statistical" and dropped whole under
        "radius"."""
        method, p0, p1 = self._check_filter(method, k, std_ratio, min_neighbours, radius2)
        self._check_output(output)
        self._check_invalid(invalid)
        frames, is_float, on_device = self._check_frames(frames)
        voxel, origin = self._check_voxel(is_float, voxel, origin, "filter")
        attrs = flat = None
        if attributes is not None:
            attributes = list(attributes)
            floats = [str(a.dtype if hasattr(a, "dtype") else np.asarray(a).dtype).replace("torch.", "") in ("float32", "float64")
                      for a in attributes]
            if any(floats) and not all(floats):
                raise ValueError("the attributes of a call are all integer (uint8 / uint16) or all float")
            # float values pass the checks as under a scale; nothing is quantised here
            attrs = self._check_attributes(frames, attributes, self._device, 1.0 if any(floats) else None, np.dtype(np.uint8))
            attrs = [a.src if isinstance(a, _Attr) else a for a in attrs]
            flat = [getattr(a, "ndim", 2) == 1 for a in attributes]

        def result(kept, kept_attrs, mask, report):
            out = (kept,) if attrs is None else (kept, kept_attrs)
            if return_mask:
                out += (mask,)
            if return_report:
                out += (report,)
            return out[0] if len(out) == 1 else out
        nb = len(frames)
        if nb == 0:
            return result([], [], [], [])
        statistical = method == "statistical"
        attrs_on_device = attrs is not None and isinstance(attrs[0], torch.Tensor)
        caller = torch.cuda.current_stream(self.rt.device) if on_device or attrs_on_device else None
        with self._lock, self.rt as rt:
            front = self._front(rt, frames, is_float, on_device, caller, "GeometryCodec.filter", 0, voxel, origin, invalid == "drop")
            if attrs_on_device:
                rt.stream.wait_stream(caller)
            points, kept_points = [0] * nb, [0] * nb
            sums = [(0, 0, 0)] * nb
            thresholds = [Runtime.OUTLIER_KEEP_ALL] * nb
            if front.n_keep == 0:
                mask = torch.zeros(front.n, dtype=torch.uint8, device=rt.device)
                kept_rows, ends = None, [0] * (nb + 1)
            else:
                if statistical:
                    scores, sums = rt.outlier_scores_frames(front.keys, nb, p0)      # the call's synchronisation for the threshold
                    thresholds = [Runtime.outlier_threshold(cnt, s1, s2, p1) for s1, s2, cnt in sums]
                    keep, counts = rt.outlier_mask_frames(front.keys, nb, scores, thresholds)
                    points = [cnt for _, _, cnt in sums]
                else:
                    keep, counts = rt.outlier_radius_frames(front.keys, nb, p0, p1)
                mask, kept_rows, ends = rt.outlier_compact_rows(self._input_rows(rt, front), keep, front.offsets.data_ptr(), nb)
                rt.sync()      # the sizes of the result
                ends = ends.cpu().tolist()
                if statistical:
                    kept_points = counts.cpu().tolist()
                else:
                    points, kept_points = (list(c) for c in zip(*counts.cpu().tolist()))
            host_mask = None
            if not on_device or (attrs is not None and not attrs_on_device) or (return_mask and output == "numpy"):
                host_mask = _split(mask.cpu().numpy().view(np.bool_), front.sizes)

            def take(a, f):
                """the kept rows of frame f's array a, where it lies; then where `output` wants it"""
                if isinstance(a, torch.Tensor):
                    a2 = a if a.dim() == 2 else a[:, None]
                    if a2.shape[1] > 1 and a2.stride(1) != 1:
                        a2 = a2.contiguous()
                    got = a2[:0] if ends[f + 1] == ends[f] else rt.take_rows(a2, kept_rows[ends[f]:ends[f + 1]])
                    got = got.reshape((-1,) + tuple(a.shape[1:]))
                    return got if output == "device" else got.cpu().numpy()
                got = a[host_mask[f]]
                return rt.to_device(got) if output == "device" else got
            kept = [take(a, f) for f, a in enumerate(frames)]
            kept_attrs = None if attrs is None else [take(a[:, 0] if flat[f] else a, f) for f, a in enumerate(attrs)]
            masks = None
            if return_mask:
                masks = host_mask if output == "numpy" else _split(mask.view(torch.bool), front.sizes)
            report = None
            if return_report:
                report = []
                for f in range(nb):
                    rep = {"points": int(points[f]), "kept": int(kept_points[f]), "rows_kept": int(ends[f + 1] - ends[f])}
                    if statistical:
                        rep.update(k_eff=min(p0, int(points[f])), S1=int(sums[f][0]), S2=int(sums[f][1]), threshold=int(thresholds[f]))
                    report.append(rep)
            rt.sync()      # a device result may be read from the caller's stream at once
            return result(kept, kept_attrs, masks, report)

    @staticmethod
    def _check_cluster(radius2, min_neighbours, min_points):
        """the rule's keywords of cluster -> (radius2, m, min_points) as Python ints"""
        if radius2 is None:
            raise ValueError("cluster needs radius2=, the squared radius in lattice units (an integer in 0 .. 4096)")
        for name, v, lo, hi, rng in (("radius2", radius2, 0, 4096, "0 .. 4096 (squared lattice units)"),
                                     ("min_neighbours", min_neighbours, 0, 31, "0 .. 31"),
                                     ("min_points", min_points, 1, 1 << 27, "1 .. 2^27")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer in {rng}, got {v!r}")
            if not lo <= v <= hi:
                raise ValueError(f"{name} must be an integer in {rng}, got {v!r}")
        return int(radius2), int(min_neighbours), int(min_points)

    def cluster(self, frames, radius2=None, min_neighbours=0, min_points=1, return_report=False, output="numpy", *, voxel=None,
                origin=(0.0, 0.0, 0.0), invalid="raise"):
        """DBSCAN clusters of every frame, on the device (include/pcc.h has the rule) -> `labels`, one int32 [n_f] per
        frame, row i the label of INPUT row i; (labels, report) with return_report.
        The rule runs per frame over the frame's distinct lattice points: a point is a core point iff at least
        min_neighbours (0 .. 31) OTHER points lie within radius2 (an integer in 0 .. 4096, squared lattice units, required);
        core points within radius2 of each other share a cluster; any other point joins its nearest core point within
        radius2 (the Morton-first among equidistant ones) or is noise; a cluster of fewer than min_points (1 .. 2^27)
        points is noise as a whole.  Clusters are numbered by size, largest first (equal sizes by their Morton-first
        point), noise is -1: frames[f][labels[f] == 0] is the subject, frames[f][labels[f] >= 0] the frame without
        small debris.  min_neighbours=0 is plain Euclidean clustering (connected components).  The result depends on
        the point set alone.  Duplicate rows share their point's label; a row dropped under invalid="drop" gets -1.
        A bool or a value of the wrong type: TypeError; a value out of range: ValueError naming the keyword.  Coarser
        radii: cluster coarser points (p >> k).
        frames: int16 / int32 lattice frames, or float32 frames with voxel= / origin= / invalid= exactly as compress
        quantises them; numpy or torch, all on the host or all on this codec's device.
        return_report: per frame a dict of Python ints, "points" (distinct), "core", "clusters", "noise" (distinct
        points), and "sizes", the clusters' sizes in label order.  output: "numpy" arrays, or "device": tensors on this
        codec's device.  An empty frame gives an empty array; a frame of one point is one cluster of size 1 at
        min_neighbours=0 and noise above."""
        radius2, m, min_points = self._check_cluster(radius2, min_neighbours, min_points)
        self._check_output(output)
        self._check_invalid(invalid)
        frames, is_float, on_device = self._check_frames(frames)
        voxel, origin = self._check_voxel(is_float, voxel, origin, "cluster")
        nb = len(frames)
        if nb == 0:
            return ([], []) if return_report else []
        caller = torch.cuda.current_stream(self.rt.device) if on_device else None
        with self._lock, self.rt as rt:
            front = self._front(rt, frames, is_float, on_device, caller, "GeometryCodec.cluster", 0, voxel, origin, invalid == "drop")
            counts, sizes = [[0, 0, 0, 0]] * nb, [[] for _ in range(nb)]
            if front.n_keep == 0:
                rows = torch.full((front.n,), -1, dtype=torch.int32, device=rt.device)
            else:
                labels, d_sizes, d_counts = rt.cluster_frames(front.keys, nb, m, radius2, min_points, want_sizes=return_report)
                index = self._input_rows(rt, front)
                rows = torch.where(index >= 0, labels[index.clamp(min=0).long()], torch.full_like(index, -1))
                if return_report:
                    counts = rt._u64_rows(d_counts)      # the call's synchronisation for the counts
                    firsts = _ends([c[0] for c in counts])      # where every frame's distinct points, and its sizes, begin
                    live = [d_sizes[firsts[f]:firsts[f] + counts[f][2]] for f in range(nb)]
                    sizes = _split(torch.cat(live).cpu().numpy().view(np.uint32).tolist(), [c[2] for c in counts])
            out = _frames_out(rt, rows, front.sizes, output == "numpy")
        if not return_report:
            return out
        return out, [{"points": int(c[0]), "core": int(c[1]), "clusters": int(c[2]), "noise": int(c[3]), "sizes": list(s)}
                     for c, s in zip(counts, sizes)]

    @staticmethod
    def _check_normals(frames, normals, device=None):
        """given normals: one finite float32 [n_f, 3] array per frame, all on the host or all tensors on `device` (the
        codec's, as normals(output="device") returns them).  Device tensors are not read here: _device_normals checks
        that they are finite, on the codec's stream."""
        normals = list(normals)
        if len(normals) != len(frames):
            raise ValueError(f"{len(normals)} normal arrays for {len(frames)} frames")
        out, places = [], []
        for f, (a, p) in enumerate(zip(normals, frames)):
            on_device = isinstance(a, torch.Tensor) and a.device.type != "cpu"
            if on_device:
                if device is None or a.device != device:
                    raise ValueError(f"frame {f}: normals on {a.device}, this codec runs on {device}")
                a = a.detach()
            elif isinstance(a, torch.Tensor):
                a = a.detach().numpy()
            else:
                a = np.asarray(a)
            places.append(on_device)
            if places[-1] != places[0]:
                raise ValueError(f"frame {f}: normals on the {'device' if on_device else 'host'}, frame 0's on the "
                                 f"{'device' if places[0] else 'host'}: the normals of a call are all on the host or all on "
                                 "the device")
            if str(a.dtype).replace("torch.", "") != "float32":
                raise TypeError(f"frame {f}: expected float32 normals, got {a.dtype}")
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"frame {f}: expected normals of shape [n, 3], got {tuple(a.shape)}")
            if a.shape[0] != p.shape[0]:
                raise ValueError(f"frame {f}: {a.shape[0]} normals for {p.shape[0]} points")
            if not on_device and not np.isfinite(a).all():
                raise ValueError(f"frame {f}: non-finite normal")
            out.append(a if on_device else np.ascontiguousarray(a))
        return out

    @staticmethod
    def _device_normals(rt, given, caller):
        """given normals on the device -> one float32 [n, 3] tensor of the call's rows, behind the caller's stream; a
        non-finite one raises ValueError naming its frame (one flag per frame, one read-back)"""
        rt.stream.wait_stream(caller)
        finite = torch.stack([torch.isfinite(a).all() for a in given]).tolist()
        if not all(finite):
            raise ValueError(f"frame {finite.index(False)}: non-finite normal")
        return torch.cat(given, 0).contiguous()

    def distortion(self, frames_a, frames_b, attributes_a=None, attributes_b=None, peak=None, normals_a=None, normal_k=16, *,
                   attribute_scale=None, attribute_dtype=None):
        """The D1 (point-to-point) distortion between two sequences of lattice frames, frame by frame, by exact nearest
        neighbours on the device (pcc_nn_frames; include/pcc.h has the rule) -> one dict per frame:

            points_a, points_b     the rows given (duplicates count, as pc_error counts them)
            mse_ab, mse_ba         mean over the rows of one side of the squared distance to the nearest point of the
                                   other side, in lattice units: integer sum / count, in float64
            max_ab, max_ba         the largest such squared distance, an int
            d1_psnr                10 log10(3 peak^2 / max(mse_ab, mse_ba)) (metrics.d1_psnr's formula), inf when both
                                   are 0, None when peak is None
            attr_mse_ab, attr_mse_ba   with attributes: per channel, the mean squared difference between a row's value
                                   and the value of its nearest point of the other side (Morton-first among equidistant)
            d2_mse_ab, d2_mse_ba   with normals_a: the D2 (point-to-plane) figures — mean over the rows of one side of
                                   the squared projection of the error vector to the nearest point of the other side
                                   onto the normal of the pair's A point, float64
            d2_psnr                10 log10(3 peak^2 / max(d2_mse_ab, d2_mse_ba)), inf and None as d1_psnr

        frames_a, frames_b: as compress takes them, int16 / int32 only, numpy or torch, all on the host or all on this
        codec's device, the same number on both sides.  float32 frames raise TypeError: pass lattice points — what
        compress was given, or decompress without voxel= returns; metric distances are these times voxel^2.  A frame
        pair with points on one side and none on the other raises ValueError naming the frame; two empty frames give
        0.0 and inf.  Cells of a level of detail compare as their centres: (cells << k) + ((1 << k) >> 1).
        attributes_a, attributes_b: uint8 / uint16 [n] or [n, c] per frame, as compress takes them — host arrays or
        tensors on this codec's device (both sides in one place), or float32 / float64 with attribute_scale= and
        attribute_dtype= as compress reads them — dtype and channel count equal per frame pair; both sides must then be
        free of duplicate points (ValueError naming the frame): the typical call compares a lossless decode with a lossy
        one.  Device attributes are widened and brought into the sorted order in one pass (pcc_attr_stage_frames).
        normals_a: only side A (the original) carries normals, as with pc_error -n.  "estimate": the normals of A's
        distinct points from their normal_k (3 .. 32) nearest neighbours, as normals() gives them; A may hold duplicates,
        a frame of A with 1 or 2 distinct points raises ValueError.  Or one finite float32 [n_f, 3] array per frame, all
        host arrays or all tensors on this codec's device (what normals(output="device") returns), row i the normal of
        row i of A, used as given: A must then be free of duplicate points; a non-finite normal raises ValueError naming
        the frame."""
        fa, dev_a, fb, dev_b = self._check_two_sides(frames_a, frames_b, "distortion",
                                                     "; metric distances are lattice distances times voxel^2")
        if (attributes_a is None) != (attributes_b is None):
            raise ValueError("distortion: attributes on one side only")
        if peak is not None and not (isinstance(peak, (int, float, np.integer, np.floating)) and not isinstance(peak, bool)
                                     and np.isfinite(peak) and peak > 0):
            raise ValueError(f"distortion: peak must be a positive number (grid extent - 1), got {peak!r}")
        attrs_a = attrs_b = None
        scale, attr_dtype = self._check_attribute_scale(attribute_scale, attribute_dtype, attributes_a is not None)
        if attributes_a is not None:
            attrs_a = self._check_attributes(fa, attributes_a, self._device, scale, attr_dtype)
            attrs_b = self._check_attributes(fb, attributes_b, self._device, scale, attr_dtype)
            places = [self._staged(x) and x[0].on_device for x in (attrs_a, attrs_b)]
            if attrs_a and places[0] != places[1]:
                raise ValueError(f"frame 0: attributes_a on the {'device' if places[0] else 'host'}, attributes_b on the "
                                 f"{'device' if places[1] else 'host'}: the attributes of a call are all on the host or all "
                                 "on the device")
            for f, (a, b) in enumerate(zip(attrs_a, attrs_b)):
                if a.dtype != b.dtype or a.shape[1] != b.shape[1]:
                    raise ValueError(f"frame {f}: {a.dtype} attributes of {a.shape[1]} channels against {b.dtype} of "
                                     f"{b.shape[1]}: dtype and channel count must be equal")
        given = None
        if isinstance(normals_a, str):
            if normals_a != "estimate":
                raise ValueError(f"normals_a must be 'estimate' or one float32 [n, 3] array per frame, got {normals_a!r}")
            normal_k = self._check_k(normal_k, "normal_k")
        elif normals_a is not None:
            given = self._check_normals(fa, normals_a, self._device)
        nb = len(fa)
        sizes_a = [int(a.shape[0]) for a in fa]
        sizes_b = [int(b.shape[0]) for b in fb]
        for f, (na, nr) in enumerate(zip(sizes_a, sizes_b)):
            if (na == 0) != (nr == 0):
                raise ValueError(f"frame {f}: {na} points against {nr}: the distance to an empty set is undefined")
        if nb == 0:
            return []
        ab = ba = [[0, 0, 0]] * nb
        sse_ab = sse_ba = None
        d2_ab = d2_ba = [0.0] * nb
        if sum(sizes_a):
            given_on_device = bool(given) and isinstance(given[0], torch.Tensor)
            attrs_on_device = self._staged(attrs_a) and attrs_a[0].on_device
            caller = torch.cuda.current_stream(self.rt.device) if dev_a or attrs_on_device or given_on_device else None
            with self._lock, self.rt as rt:
                if given_on_device:
                    given = self._device_normals(rt, given, caller)
                front_a = self._front(rt, fa, False, dev_a, caller, "GeometryCodec.distortion")
                front_b = self._front(rt, fb, False, dev_b, caller, "GeometryCodec.distortion")
                if attrs_a is not None:
                    self._refuse_duplicates(front_a, "frames_a")
                    self._refuse_duplicates(front_b, "frames_b")
                if given is not None:
                    self._refuse_duplicates(front_a, "frames_a")
                elif normals_a is not None:
                    self._refuse_few(front_a, "frames_a")
                want_row = attrs_a is not None or normals_a is not None
                _, row_ab, ab = rt.nn_frames(front_a.sorted_keys, front_b.keys, nb, want_dist=False, want_row=want_row)
                _, row_ba, ba = rt.nn_frames(front_b.sorted_keys, front_a.keys, nb, want_dist=False, want_row=want_row)
                if normals_a is not None:
                    d2_ab, d2_ba = self._d2_sums(rt, front_a, front_b, row_ab, row_ba, given, normal_k)
                if attrs_a is not None:
                    dtype, channels = self._common_format(attrs_a)
                    statuses = []
                    va = self._sorted_any(rt, attrs_a, front_a.perm, dtype, channels, caller, scale, statuses)
                    vb = self._sorted_any(rt, attrs_b, front_b.perm, dtype, channels, caller, scale, statuses)
                    sse_ab = rt.nn_attr_sse_frames(front_a.sorted_keys, row_ab, va, vb, nb)
                    sse_ba = rt.nn_attr_sse_frames(front_b.sorted_keys, row_ba, vb, va, nb)
                    for status in statuses:      # behind the synchronisation of the sums
                        self._check_stage_status(status, "GeometryCodec.distortion")
        elif attrs_a is not None:
            sse_ab = sse_ba = [[0] * 4] * nb
        report = []
        for f in range(nb):
            (ca, sa, ma), (cb, sb, mb) = ab[f], ba[f]
            rep = {"points_a": sizes_a[f], "points_b": sizes_b[f],
                   "mse_ab": float(sa) / float(ca) if ca else 0.0, "mse_ba": float(sb) / float(cb) if cb else 0.0,
                   "max_ab": int(ma), "max_ba": int(mb)}
            worst = max(rep["mse_ab"], rep["mse_ba"])
            rep["d1_psnr"] = None if peak is None else (float("inf") if worst == 0.0 else
                                                       float(10.0 * np.log10(3.0 * float(peak) ** 2 / worst)))
            if normals_a is not None:
                rep["d2_mse_ab"] = d2_ab[f] / float(ca) if ca else 0.0
                rep["d2_mse_ba"] = d2_ba[f] / float(cb) if cb else 0.0
                worst = max(rep["d2_mse_ab"], rep["d2_mse_ba"])
                rep["d2_psnr"] = None if peak is None else (float("inf") if worst == 0.0 else
                                                           float(10.0 * np.log10(3.0 * float(peak) ** 2 / worst)))
            if attrs_a is not None:
                c = attrs_a[f].shape[1]
                rep["attr_mse_ab"] = [float(s) / float(ca) if ca else 0.0 for s in sse_ab[f][:c]]
                rep["attr_mse_ba"] = [float(s) / float(cb) if cb else 0.0 for s in sse_ba[f][:c]]
            report.append(rep)
        return report

    @staticmethod
    def _d2_sums(rt, front_a, front_b, row_ab, row_ba, given, normal_k):
        """the per-frame sums of the D2 projections of both directions: the normals of A's distinct points — estimated,
        or `given` per input row of a duplicate-free A and brought into the order of its sorted keys — then one
        pcc_nn_d2_frames per direction, the normal of a pair always that of its A point"""
        nb = front_a.nb
        of_query = None      # A -> B: query i of the sorted keys is distinct row i, unless A holds duplicates
        if given is None:
            normals = rt.knn_frames(front_a.keys, nb, normal_k)[3]
            if front_a.n_unique != front_a.n_keep:
                of_query = rt.lookup(front_a.keys, front_a.sorted_keys)
        elif isinstance(given, torch.Tensor):      # the call's rows on the device already (_device_normals)
            normals = rt.gather_rows(given, front_a.perm)
        else:
            host = torch.empty((front_a.n, 3), dtype=torch.float32, pin_memory=True)
            np.concatenate(given, axis=0, out=host.numpy())
            normals = rt.gather_rows(rt.to_device(host), front_a.perm)
        _, d2_ab = rt.nn_d2_frames(front_a.sorted_keys, row_ab, front_b.keys, normals, nb, of_query)
        _, d2_ba = rt.nn_d2_frames(front_b.sorted_keys, row_ba, front_a.keys, normals, nb, row_ba)
        return d2_ab, d2_ba

    @staticmethod
    def _refuse_duplicates(front, side):
        """ValueError naming the first frame of `side` whose sorted keys hold a duplicate (the distinct count says so)"""
        if front.n_unique == front.n_keep:
            return
        sizes, counts = front.sizes, GeometryCodec._frame_counts(front.keys, front.nb)
        f = next(f for f, (n, u) in enumerate(zip(sizes, counts)) if u < n)
        raise ValueError(f"frame {f}: {sizes[f] - int(counts[f])} duplicate points in {side}: attributes are compared point by "
                         "point, so both sides must be free of duplicates (a decoded frame is)")

    def transfer(self, frames_from, attributes, frames_to, output="numpy", return_counts=False, *, attribute_scale=None,
                 attribute_dtype=None):
        """The attributes of one geometry carried onto another (recolouring), frame by frame on the device
        (pcc_attr_transfer_frames; include/pcc.h has the rule) -> one array per frame, row i the value of row i of
        frames_to[f] as given: [n_to] for attributes given as [n], [n_to, c] otherwise, in the attributes' dtype.

        Every source row is assigned to its nearest target point and every target takes the rounded mean
        (sum + count // 2) // count of the rows assigned to it — the merge rule of compress for duplicate points; a target
        that no source row chose takes the merged value of its nearest source point.  Nearest is exact, ties go to the
        Morton-first point (the rule of distortion).  Rows of frames_to that share a point share its value.
        frames_from, frames_to: as distortion takes them, int16 / int32, numpy or torch, all on the host or all on this
        codec's device, the same number on both sides; float32 frames raise TypeError.  attributes: uint8 / uint16
        [n] or [n, c] per frame of frames_from, as compress takes them: host arrays, tensors on this codec's device, or
        float32 / float64 values with attribute_scale= (and attribute_dtype=), the result then in the dtype they become.
        A frame with targets and no source raises ValueError naming the frame; a frame without targets gives [0] / [0, c].
        output: "numpy" arrays, or "device": views of one tensor on this codec's device.  return_counts=True:
        (values, counts), counts[f] a uint32 [n_to]: the source rows assigned to the row's point, 0 where the value is
        the fallback."""
        self._check_output(output)
        ff, dev_f, ft, dev_t = self._check_two_sides(frames_from, frames_to, "transfer")
        attributes = list(attributes)
        flat = [(a.dim() if isinstance(a, torch.Tensor) else np.ndim(a)) == 1 for a in attributes]
        scale, attr_dtype = self._check_attribute_scale(attribute_scale, attribute_dtype, True)
        attrs = self._check_attributes(ff, attributes, self._device, scale, attr_dtype)
        nb = len(ff)
        sizes_f = [int(a.shape[0]) for a in ff]
        sizes_t = [int(a.shape[0]) for a in ft]
        for f, (ns, nt) in enumerate(zip(sizes_f, sizes_t)):
            if nt and not ns:
                raise ValueError(f"frame {f}: {nt} points against an empty source: there is no value to transfer")
        if nb == 0:
            return ([], []) if return_counts else []
        to_host = output == "numpy"
        dtype, channels = self._common_format(attrs)
        if sum(sizes_t) == 0:
            values = torch.empty((0, channels), dtype=torch.uint8 if dtype == np.uint8 else torch.uint16,
                                 device="cpu" if to_host else self.rt.device)
            counts = torch.empty((0,), dtype=torch.int32, device=values.device)
            if to_host:
                values, counts = values.numpy(), counts.numpy()
            values, counts = _split(values, sizes_t), _split(counts, sizes_t)
        else:
            attrs_on_device = self._staged(attrs) and attrs[0].on_device
            caller = torch.cuda.current_stream(self.rt.device) if dev_f or attrs_on_device else None
            with self._lock, self.rt as rt:
                front_f = self._front(rt, ff, False, dev_f, caller, "GeometryCodec.transfer")
                front_t = self._front(rt, ft, False, dev_t, caller, "GeometryCodec.transfer")
                _, row_st, _ = rt.nn_frames(front_f.sorted_keys, front_t.keys, nb, want_dist=False)
                _, row_ts, _ = rt.nn_frames(front_t.keys, front_f.keys, nb, want_dist=False)
                statuses = []
                sv = self._sorted_any(rt, attrs, front_f.perm, dtype, channels, caller, scale, statuses)
                distinct, cnt = rt.attr_transfer_frames(front_f.sorted_keys, front_f.rows, front_f.n_unique, sv, row_st, row_ts,
                                                        nb, want_count=return_counts)
                index = self._input_rows(rt, front_t)      # of every target row as given
                values = _frames_out(rt, rt.gather_rows(distinct, index), sizes_t, to_host)
                counts = _frames_out(rt, rt.gather_rows(cnt, index), sizes_t, to_host) if return_counts else None
                for status in statuses:      # behind the synchronisation of _frames_out
                    self._check_stage_status(status, "GeometryCodec.transfer")
        out = []
        for v, a, one in zip(values, attrs, flat):
            v = v[:, 0] if one else v[:, :a.shape[1]]
            if a.dtype != dtype:      # a uint8 frame in a call that also holds uint16 frames
                v = v.astype(a.dtype) if to_host else v.contiguous().view(torch.uint8).reshape(v.shape + (2,))[..., 0]      # the low bytes
            out.append(v)
        if not return_counts:
            return out
        return out, [c.view(np.uint32 if to_host else torch.uint32) for c in counts]

    @staticmethod
    def _named(first, call):
        """a run of frames decoded in a call of its own: the frame an error names counts from the run's first frame"""
        try:
            return call()
        except PccError as e:
            if first:
                e.args = tuple(re.sub(r"frame (\d+):", lambda m: f"frame {int(m.group(1)) + first}:", a, count=1)
                               if isinstance(a, str) else a for a in e.args)
            raise


__all__ = ["GeometryCodec", "PccError", "MAX_FRAMES", "MAX_LOD"]
