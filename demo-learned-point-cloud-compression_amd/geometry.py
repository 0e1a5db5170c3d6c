"""GeometryCodec: lossless geometry-only coding of sequences of point sets (LiDAR sweeps) on the GPU.

Every frame becomes an independent blob of version 2 (csrc/octree2.hip), byte-identical to what the one-frame coder
(pcc_octree_encode_version, version 2) writes for np.unique(points, axis=0) of that frame alone; all frames of a call
are coded side by side by one pcc_octree_encode_frames call and decoded by one pcc_octree_decode_frames call.

    codec = GeometryCodec()
    blobs = codec.compress([pts0, pts1, ...])            # int16 / int32 [n_f, 3] in [-32768, 32767]
    frames = codec.decompress(blobs)                     # int32 [n_f, 3], Morton order (as pcc_octree_decode_dev)
    frames = codec.decompress(blobs, output="device")    # the same as views of one device tensor

One Runtime (ctx + stream) per codec; calls on the same instance are serialised, instances on different threads run
side by side.
"""
import ctypes as C
import threading

import numpy as np
import torch

from ._abi import check, PccError, PCC_E_RANGE
from .runtime import Runtime, _ptr

MAX_FRAMES = 65535      # the batch-index range of pcc_morton_keys


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

    def compress(self, frames):
        """frames: a sequence of int16 / int32 [n_f, 3] arrays -> a list of bytes, one version-2 blob per frame.
        Duplicate points are removed (as np.unique), out-of-range coordinates raise PccError (PCC_E_RANGE)."""
        frames = self._check_frames(frames)
        nb = len(frames)
        if nb == 0:
            return []
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
                return rt.octree_encode_frames(rt.empty((0,), torch.int64), nb)
            dev = rt.to_device(host)
            keys = rt.empty((n,), torch.int64)
            flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
            check(rt.lib.pcc_morton_keys_frames(rt.ctx, C.c_void_p(dev.data_ptr() + rows_at), np.dtype(dtype).itemsize, n,
                                                C.c_void_p(dev.data_ptr()), nb, _ptr(keys), _ptr(flag)),
                  "pcc_morton_keys_frames")
            rt.sort_pairs(keys)
            # duplicates (np.unique): the first row of every run of equal keys
            rows = rt.empty((n,), torch.int32)
            n_u = C.c_int64(0)
            check(rt.lib.pcc_unique_rows(rt.ctx, _ptr(rt.keys_to_coords(keys)), n, _ptr(rows), C.byref(n_u)),
                  "pcc_unique_rows")
            if int(flag.item()) != 0:      # read behind the synchronisation of pcc_unique_rows
                raise PccError(PCC_E_RANGE, "GeometryCodec.compress", "coordinate outside [-32768, 32767]")
            if n_u.value < n:
                keys = rt.gather_rows(keys, rows[:n_u.value])
            return rt.octree_encode_frames(keys, nb)

    def decompress(self, blobs, output="numpy"):
        """version-2 blobs -> a list of int32 [n_f, 3] point sets in Morton order: numpy arrays (output="numpy") or
        device tensors (output="device", on this codec's device)"""
        if output not in ("numpy", "device"):
            raise ValueError(f"output must be 'numpy' or 'device', got {output!r}")
        blobs = [bytes(b) for b in blobs]
        if len(blobs) > MAX_FRAMES:
            raise ValueError(f"{len(blobs)} blobs in one call, at most {MAX_FRAMES}")
        with self._lock, self.rt as rt:
            return rt.octree_decode_frames(blobs, device=(output == "device"))


__all__ = ["GeometryCodec", "PccError", "MAX_FRAMES"]
