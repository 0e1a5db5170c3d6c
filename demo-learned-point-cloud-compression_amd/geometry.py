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

Attributes are lossless (attribute blob version 1, csrc/attr.hip), one blob per frame beside its geometry blob; the
values of duplicate points merge to their rounded mean per channel, (sum + cnt // 2) // cnt.

Attributes at a level of detail (attribute blob version 2, csrc/attr_blob.h has the rule): the sender chooses it, and
the values of every coarser level are a prefix of that blob's bytes too.

    blobs, attr_blobs = codec.compress(frames, attributes=attrs, scalable=True)
    abytes, values = GeometryCodec.attr_lod_info(attr_blob, 2)        # host only; values == lod_info(blob, 2)[1]
    cells, attrs = codec.decompress([b[:nbytes]], [a[:abytes]], lod=2)

Row j of attrs[f] is the value of the Morton-first point of cell j: a SAMPLE of the cell, where the sender's side
compress(frames, attributes=..., lod=2) stores the cell's MEAN.  At lod 0 version 2 returns what version 1 returns.

One Runtime (ctx + stream) per codec; calls on the same instance are serialised, instances on different threads run
side by side.
"""
import ctypes as C
import re
import struct
import threading

import numpy as np
import torch

from ._abi import check, PccError, PCC_E_RANGE
from .runtime import Runtime, _ptr

MAX_FRAMES = 65535      # the batch-index range of pcc_morton_keys
MAX_LOD = 15            # levels of detail 0 .. 15 (csrc/octree2_blob.h)


class GeometryCodec:
    def __init__(self, device=0):
        self.rt = Runtime(device)
        self._lock = threading.Lock()

    def close(self):
        self.rt.close()

    @staticmethod
    def _check_frames(frames):
        out = []
        for f, a in enumerate(frames):
            a = np.asarray(a)
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"frame {f}: expected an [n, 3] array, got shape {a.shape}")
            if a.dtype not in (np.int16, np.int32):
                raise TypeError(f"frame {f}: expected int16 or int32 coordinates, got {a.dtype}")
            out.append(a)
        if len(out) > MAX_FRAMES:
            raise ValueError(f"{len(out)} frames in one call, at most {MAX_FRAMES}")
        return out

    @staticmethod
    def _check_attributes(frames, attributes):
        attributes = list(attributes)
        if len(attributes) != len(frames):
            raise ValueError(f"{len(attributes)} attribute arrays for {len(frames)} frames")
        out = []
        for f, (a, p) in enumerate(zip(attributes, frames)):
            a = np.asarray(a)
            if a.dtype not in (np.uint8, np.uint16):
                raise TypeError(f"frame {f}: expected uint8 or uint16 attributes, got {a.dtype}")
            if a.ndim == 1:
                a = a[:, None]
            if a.ndim != 2 or not 1 <= a.shape[1] <= 4:
                raise ValueError(f"frame {f}: expected attributes of shape [n] or [n, c] with 1 <= c <= 4, got {a.shape}")
            if a.shape[0] != p.shape[0]:
                raise ValueError(f"frame {f}: {a.shape[0]} attribute rows for {p.shape[0]} points")
            out.append(np.ascontiguousarray(a.astype(a.dtype.newbyteorder("<"), copy=False)))
        return out

    @staticmethod
    def _check_lod(lod):
        if not isinstance(lod, (int, np.integer)) or isinstance(lod, bool) or not 0 <= lod <= MAX_LOD:
            raise ValueError(f"lod must be an integer in 0 .. {MAX_LOD}, got {lod!r} (32768 is not a multiple of 2^16: "
                             "the cells of level 16 would not nest in a root cube)")
        return int(lod)

    @staticmethod
    def lod_info(blob, lod):
        """(bytes, cells) of level of detail `lod` of a version-2 blob: blob[:bytes] is the shortest prefix that
        decompress(..., lod=lod) reads, `cells` the rows it gives.  Host only (no GPU needed); `blob` may be a prefix
        that reaches the last needed chunk's length table."""
        return Runtime.octree_lod_info(bytes(blob), GeometryCodec._check_lod(lod))

    @staticmethod
    def attr_lod_info(attr_blob, lod):
        """(bytes, values) of level of detail `lod` of a version-2 attribute blob (compress(..., scalable=True)):
        attr_blob[:bytes] is the shortest prefix that decompress(..., lod=lod) reads, `values` the rows it gives (the
        cells of the frame's geometry at that lod).  Host only; `attr_blob` may be a prefix that reaches the last needed
        chunk's length table."""
        return Runtime.attr_lod_info(bytes(attr_blob), GeometryCodec._check_lod(lod))

    def compress(self, frames, attributes=None, lod=0, scalable=False):
        """frames: a sequence of int16 / int32 [n_f, 3] arrays -> a list of bytes, one version-2 blob per frame.
        Duplicate points are removed (as np.unique), out-of-range coordinates raise PccError (PCC_E_RANGE).
        lod = k > 0: the sender's side of a level of detail — blob f is the version-2 blob of the distinct cells
        points_f >> k (under bias 32768 >> k), which every decoder reads as those cell indices; the rows of a CELL
        merge as duplicate points do, in one merge over all input rows of the cell.
        attributes (optional): one uint8 / uint16 [n_f] or [n_f, c] array per frame (1 <= c <= 4) -> (blobs,
        attribute blobs): attribute blob f holds, losslessly, one row per decoded point of frame f (Morton order), the
        rows of duplicate points merged to their rounded mean per channel.  scalable=True: attribute blobs of version 2,
        whose coarser levels of detail are prefixes (attr_lod_info, decompress(..., lod=k)); the geometry blobs are the
        same, the default stays version 1.  With lod = k it codes the cells' means over the cells' keys."""
        lod = self._check_lod(lod)
        version = 2 if scalable else 1
        frames = self._check_frames(frames)
        attrs = None if attributes is None else self._check_attributes(frames, attributes)
        nb = len(frames)
        if nb == 0:
            return [] if attrs is None else ([], [])
        sizes = [a.shape[0] for a in frames]
        n = int(sum(sizes))
        # one upload, the rows as they come (6 or 12 B per point) behind the frame offsets; the frame index and the
        # widening to keys happen on the device (pcc_morton_keys_frames)
        dtype = np.int16 if all(a.dtype == np.int16 for a in frames) else np.int32
        offs_b = 8 * (nb + 1)
        rows_at = (offs_b + 15) // 16 * 16
        host = torch.empty(rows_at + 3 * n * np.dtype(dtype).itemsize, dtype=torch.uint8, pin_memory=True)
        h = host.numpy()
        np.cumsum([0] + sizes, out=h[:offs_b].view(np.int64))
        if n:
            np.concatenate(frames, axis=0, out=h[rows_at:].view(dtype).reshape(n, 3))
        with self._lock, self.rt as rt:
            if n == 0:
                blobs = rt.octree_encode_frames(rt.empty((0,), torch.int64), nb)
                return blobs if attrs is None else (blobs, self._encode_attributes(rt, attrs, sizes, blobs, None, None, 0, version))
            dev = rt.to_device(host)
            keys = rt.empty((n,), torch.int64)
            flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
            check(rt.lib.pcc_morton_keys_frames(rt.ctx, C.c_void_p(dev.data_ptr() + rows_at), np.dtype(dtype).itemsize, n,
                                                C.c_void_p(dev.data_ptr()), nb, _ptr(keys), _ptr(flag)),
                  "pcc_morton_keys_frames")
            perm = rt.sort_pairs(keys)
            if lod:      # a cell's keys differ in their low 3 lod bits only (the batch index above bit 48 stays)
                keys.bitwise_and_(-(1 << (3 * lod)))
            # duplicates (np.unique): the first row of every run of equal keys
            rows = rt.empty((n,), torch.int32)
            n_u = C.c_int64(0)
            check(rt.lib.pcc_unique_rows(rt.ctx, _ptr(rt.keys_to_coords(keys)), n, _ptr(rows), C.byref(n_u)),
                  "pcc_unique_rows")
            if int(flag.item()) != 0:      # read behind the synchronisation of pcc_unique_rows
                raise PccError(PCC_E_RANGE, "GeometryCodec.compress", "coordinate outside [-32768, 32767]")
            if n_u.value < n:
                keys = rt.gather_rows(keys, rows[:n_u.value])
            blobs = rt.octree_encode_frames(keys, nb, 3 * lod)
            if attrs is None:
                return blobs
            return blobs, self._encode_attributes(rt, attrs, sizes, blobs, perm, rows, n_u.value, version, keys, 3 * lod)

    @staticmethod
    def _encode_attributes(rt, attrs, sizes, blobs, perm, rows, n_unique, version=1, keys=None, key_shift=0):
        # the values as they come, frame by frame at 16-byte offsets, in one upload; the merge into Morton order
        # happens on the device from the sort's permutation and the runs of equal keys
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
        row_offsets = np.cumsum([0] + list(sizes)).tolist()
        return rt.attr_encode_frames(values, offs, formats, row_offsets, points, perm, rows, n_unique, version, keys, key_shift)

    def decompress(self, blobs, attr_blobs=None, output="numpy", lod=0):
        """version-2 blobs -> a list of int32 [n_f, 3] point sets in Morton order: numpy arrays (output="numpy") or
        device tensors (output="device", on this codec's device).  With attr_blobs (compress(..., attributes=...)):
        (point sets, attributes), attributes[f] an [n_f, c] array in its original dtype, row i belonging to point i; an
        attribute blob decodes only with the geometry blob of its own frame (another point count raises PccError).
        lod = k > 0: blobs or prefixes of them (lod_info) -> the distinct cell indices points >> k of every frame, int32
        [cells, 3] in Morton order (corner of a cell c << k, centre (c << k) + ((1 << k) >> 1)); with attr_blobs of
        version 2 (compress(..., scalable=True)), or prefixes of them (attr_lod_info): attributes[f] is [cells, c], row j
        the value of the Morton-first point of cell j.  Versions may be mixed at lod 0; an attribute blob of version 1
        at lod > 0 raises ValueError."""
        if isinstance(attr_blobs, str):      # decompress(blobs, "device"), as before attributes
            attr_blobs, output = None, attr_blobs
        if output not in ("numpy", "device"):
            raise ValueError(f"output must be 'numpy' or 'device', got {output!r}")
        lod = self._check_lod(lod)
        blobs = [bytes(b) for b in blobs]
        if len(blobs) > MAX_FRAMES:
            raise ValueError(f"{len(blobs)} blobs in one call, at most {MAX_FRAMES}")
        if attr_blobs is not None:
            attr_blobs = [bytes(b) for b in attr_blobs]
            if len(attr_blobs) != len(blobs):
                raise ValueError(f"{len(attr_blobs)} attribute blobs for {len(blobs)} geometry blobs")
            v1 = [len(b) > 1 and b[1] == 1 for b in attr_blobs]
            if lod and any(v1):
                raise ValueError(f"frame {v1.index(True)}: attributes of blob version 1 cannot be decoded at lod > 0: it "
                                 "is one predictive stream in full-resolution Morton order, so neither its bytes nor "
                                 "its decoding can be cut; store version 2 (compress(..., scalable=True)) or ship "
                                 "coarse attributes with compress(frames, attributes=..., lod=k)")
        with self._lock, self.rt as rt:
            # version 2 reads the cells where the geometry decode left them: on the device
            on_device = attr_blobs is not None and not all(v1)
            frames = rt.octree_decode_frames(blobs, device=(output == "device" or on_device), lod=lod)
            if attr_blobs is None:
                return frames
            if all(v1):
                return frames, rt.attr_decode_frames(attr_blobs, points=[f.shape[0] for f in frames],
                                                     device=(output == "device"))
            cells = frames
            if output == "numpy":      # one copy of the call's cells to the host, split as the device tensor is
                host = torch.cat(cells).cpu().numpy()
                ends = np.cumsum([0] + [c.shape[0] for c in cells])
                frames = [host[a:b] for a, b in zip(ends[:-1], ends[1:])]
            attrs = [None] * len(blobs)
            f = 0
            while f < len(blobs):      # runs of frames of one version, each in one call
                g = f
                while g < len(blobs) and v1[g] == v1[f]:
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
