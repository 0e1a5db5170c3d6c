"""Runtime: one pcc_ctx (device + HIP stream + scratch arena) with tensor-level
wrappers around the C-ABI.

torch is used here for what the task allows it for — device memory (caching
allocator), streams and host<->device copies.  Every computation on device
tensors goes through libpcc_hip.so; nothing here computes with torch ops.
One Runtime per in-flight compress()/decompress() call (the reference runs up
to three concurrent calls, sender/encoder/encoder.py:50).
"""
import ctypes as C
import math
import os
import struct
import threading
from typing import NamedTuple

import numpy as np
import torch

from . import _abi
from ._abi import check, PccError

_tls = threading.local()

# Host thread pools must fit the CPU share of the box (see _abi.host_cpu_budget): the codec's
# host side is a handful of short tensor conversions, so a small intra-op pool is enough.
HOST_THREADS = int(os.environ.get("PCC_HOST_THREADS", "0")) or min(8, _abi.host_cpu_budget())
if torch.get_num_threads() > HOST_THREADS:
    torch.set_num_threads(HOST_THREADS)


def current():
    rt = getattr(_tls, "rt", None)
    if rt is None:
        raise RuntimeError("no active pcc Runtime on this thread (use `with runtime:`)")
    return rt


def _ptr(t):
    """device pointer of a tensor (NULL for None / empty).  A host tensor here would make a kernel
    dereference a host address — refuse it before it reaches the GPU."""
    if t is None or t.numel() == 0:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise TypeError("device tensor expected, got a host tensor")
    if not t.is_contiguous():
        raise TypeError("contiguous device tensor expected")
    return C.c_void_p(t.data_ptr())


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


class Runtime:
    def __init__(self, device=0, stream=None):
        if not torch.cuda.is_available():
            raise RuntimeError("pcc Runtime needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = _abi.lib()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)
        self.ctx = self.lib.pcc_create(device, C.c_void_p(self.stream.cuda_stream))
        if not self.ctx:
            raise PccError(-2, "pcc_create", self.lib.pcc_last_error().decode())
        self._stream_cm = None
        self._prev = None

    @classmethod
    def adopt(cls, ctx, stream, device):
        """Runtime view of a ctx owned by someone else (a pcc_codec): same helpers / profiler,
        close() leaves the ctx alone"""
        self = cls.__new__(cls)
        self.lib = _abi.lib()
        self.device = device
        self.stream = stream
        self.ctx = ctx
        self._owned = False
        self._stream_cm = None
        self._prev = None
        return self

    def close(self):
        if self.ctx and getattr(self, "_owned", True):
            self.lib.pcc_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # `with rt:` makes rt the thread's active runtime and its stream torch's current stream
    def __enter__(self):
        self._prev = getattr(_tls, "rt", None)
        _tls.rt = self
        self._stream_cm = torch.cuda.stream(self.stream)
        self._stream_cm.__enter__()
        return self

    def __exit__(self, *exc):
        self._stream_cm.__exit__(*exc)
        _tls.rt = self._prev
        return False

    # ------------------------------------------------------------ helpers
    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def sync(self):
        check(self.lib.pcc_sync(self.ctx), "pcc_sync")

    def to_device(self, a, dtype=None):
        """host numpy / torch -> device tensor on this runtime's stream"""
        if isinstance(a, torch.Tensor):
            t = a
        else:
            t = torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        if t.device != self.device:
            t = t.to(self.device, non_blocking=True)
        return t.contiguous()

    def timer_start(self):
        check(self.lib.pcc_timer_start(self.ctx), "pcc_timer_start")

    def timer_stop_ms(self):
        check(self.lib.pcc_timer_stop(self.ctx), "pcc_timer_stop")
        ms = C.c_float(0)
        check(self.lib.pcc_timer_elapsed_ms(self.ctx, C.byref(ms)), "pcc_timer_elapsed_ms")
        return ms.value

    # ------------------------------------------------------------ per-launch profiler
    def prof_enable(self, on=True, reserve=0, only=None, rows=-1):
        """reserve > 1 pre-creates that many event pairs (keeps event creation out of the timed region);
        only / rows: bracket just the entry points whose op name starts with `only` (and whose output row
        count is `rows`) — every event pair is a few microseconds of bubble on the stream"""
        check(self.lib.pcc_prof_only(self.ctx, only.encode() if only else None, int(rows)), "pcc_prof_only")
        check(self.lib.pcc_prof_enable(self.ctx, max(int(reserve), 1) if on else 0), "pcc_prof_enable")

    def prof_records(self):
        """[(op, ms, (d0,d1,d2,d3)), ...] of every C-ABI call since prof_enable (synchronises)"""
        out = []
        name = C.create_string_buffer(64)
        ms = C.c_float(0)
        dims = (C.c_int64 * 4)()
        for i in range(self.lib.pcc_prof_count(self.ctx)):
            check(self.lib.pcc_prof_get(self.ctx, i, name, 64, C.byref(ms), dims), "pcc_prof_get")
            out.append((name.value.decode(), float(ms.value), tuple(int(d) for d in dims)))
        return out

    def exclusive_scan(self, t, inplace=False):
        """exclusive prefix sum of an int32 / uint32 vector (mod 2^32): returns (scan, total tensor [1])"""
        n = t.shape[0]
        out = t if inplace else self.empty((n,), torch.int32)
        total = self.empty((1,), torch.int32)
        check(self.lib.pcc_exclusive_scan_u32(self.ctx, _ptr(t), _ptr(out), n, _ptr(total)), "pcc_exclusive_scan_u32")
        return out, total

    def count_nonneg(self, t):
        cnt = C.c_int64(0)
        check(self.lib.pcc_count_nonneg(self.ctx, _ptr(t), t.numel(), C.byref(cnt)), "pcc_count_nonneg")
        return cnt.value

    # ------------------------------------------------------------ keys / order
    def morton_keys(self, coords):
        n = coords.shape[0]
        keys = self.empty((n,), torch.int64)
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(self.lib.pcc_morton_keys(self.ctx, _ptr(coords), n, _ptr(keys), _ptr(flag)), "pcc_morton_keys")
        if n and int(flag.item()) != 0:
            raise PccError(_abi.PCC_E_RANGE, "pcc_morton_keys",
                           "coordinate outside [-32768,32767] or batch index outside [0,65534]")
        return keys

    def keys_to_coords(self, keys):
        n = keys.shape[0]
        coords = self.empty((n, 4), torch.int32)
        check(self.lib.pcc_keys_to_coords(self.ctx, _ptr(keys), n, _ptr(coords)), "pcc_keys_to_coords")
        return coords

    def morton_keys_frames_f32(self, xyz_ptr, n, offsets_ptr, n_frames, voxel, origin, drop=False):
        """keys of n float32 rows at device address xyz_ptr, quantised by the metric rule of include/pcc.h
        (pcc_morton_keys_frames_f32); offsets_ptr: the n_frames + 1 frame offsets (int64) on the device.  Returns (keys,
        status): status an int32 [2] device tensor, [0] bit 0 = off the grid, bit 1 = non-finite, [1] = rows dropped
        (drop=True).  Does not synchronise."""
        keys = self.empty((n,), torch.int64)
        status = torch.zeros(2, dtype=torch.int32, device=self.device)
        check(self.lib.pcc_morton_keys_frames_f32(self.ctx, C.c_void_p(xyz_ptr), n, C.c_void_p(offsets_ptr), n_frames,
                                                  float(voxel), (C.c_float * 3)(*[float(v) for v in origin]),
                                                  1 if drop else 0, _ptr(keys), _ptr(status)), "pcc_morton_keys_frames_f32")
        return keys, status

    def rows_index(self, perm, n_keep, run_starts, n_unique, offsets_ptr, first_run, n_frames):
        """int32 [n] device tensor: the decoded row of its frame that every input row of a compress call became, -1 for
        a dropped row (pcc_rows_index).  perm: sort_pairs' permutation of the call's n keys; run_starts / n_unique:
        pcc_unique_rows over the first n_keep sorted keys; offsets_ptr: the frame offsets on the device; first_run: an
        int64 [n_frames] device tensor, the points of the frames in front of each frame."""
        n = perm.shape[0]
        index = self.empty((n,), torch.int32)
        check(self.lib.pcc_rows_index(self.ctx, _ptr(perm), n, int(n_keep), _ptr(run_starts), int(n_unique),
                                      C.c_void_p(offsets_ptr), _ptr(first_run), n_frames, _ptr(index)), "pcc_rows_index")
        return index

    def points_to_metric(self, points, lod, voxel, origin):
        """int32 [n, 3] lattice points or cells of level of detail `lod` on the device -> float32 [n, 3], x = o + t v
        (pcc_points_to_metric, the rule of include/pcc.h)"""
        n = points.shape[0]
        out = self.empty((n, 3), torch.float32)
        check(self.lib.pcc_points_to_metric(self.ctx, _ptr(points), n, int(lod), float(voxel),
                                            (C.c_float * 3)(*[float(v) for v in origin]), _ptr(out)), "pcc_points_to_metric")
        return out

    def nn_frames(self, qkeys, rkeys, n_frames, want_dist=True, want_row=True):
        """exact nearest neighbours on the lattice, frame by frame (pcc_nn_frames, the rule of include/pcc.h).  qkeys:
        Morton keys of the queries on the device, any order, duplicates allowed; rkeys: the reference keys, sorted and
        distinct.  Returns (sqdist, row, stats): sqdist an int64 [n_q] device tensor holding the uint64 squared
        distances (2^64 - 1 reads as -1: a frame without a reference), row an int32 [n_q] device tensor, the row of
        rkeys of the nearest point (-1 likewise) — either None when not wanted — and stats, an [n_frames, 3] list of
        Python ints (count, sum, max per frame).  Synchronises."""
        n_q, n_r = int(qkeys.shape[0]), int(rkeys.shape[0])
        sqdist = self.empty((n_q,), torch.int64) if want_dist else None
        row = self.empty((n_q,), torch.int32) if want_row else None
        stats = self.empty((n_frames, 3), torch.int64)
        check(self.lib.pcc_nn_frames(self.ctx, _ptr(qkeys), n_q, _ptr(rkeys), n_r, int(n_frames), _ptr(sqdist), _ptr(row),
                                     _ptr(stats)), "pcc_nn_frames")
        return sqdist, row, self._u64_rows(stats)

    def nn_attr_sse_frames(self, qkeys, row, a, b, n_frames):
        """per frame and channel the sum of (a[i] - b[row[i]])^2 over the frame's queries (pcc_nn_attr_sse_frames): a
        [n_q, c] and b [n_r, c] uint8 or uint16 device tensors in the order of qkeys and of the reference keys that gave
        `row`.  Returns an [n_frames, c] list of Python ints.  Synchronises."""
        if a.dtype != b.dtype or a.dtype not in (torch.uint8, torch.uint16) or a.dim() != 2 or b.dim() != 2 or \
                a.shape[1] != b.shape[1] or a.shape[0] != qkeys.shape[0] or row.shape[0] != qkeys.shape[0]:
            raise ValueError(f"nn_attr_sse_frames: values {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype} for "
                             f"{qkeys.shape[0]} queries")
        sse = self.empty((n_frames, int(a.shape[1])), torch.int64)
        check(self.lib.pcc_nn_attr_sse_frames(self.ctx, _ptr(qkeys), _ptr(row), int(qkeys.shape[0]), _ptr(a), _ptr(b),
                                              int(b.shape[0]), a.element_size(), int(a.shape[1]), int(n_frames), _ptr(sse)),
              "pcc_nn_attr_sse_frames")
        return self._u64_rows(sse)

    def attr_transfer_frames(self, skeys, sruns, n_su, svalues, row_st, row_ts, n_frames, out=None, want_count=True):
        """the values of a source side carried onto the distinct points of a target side (pcc_attr_transfer_frames, the
        rule of include/pcc.h).  skeys: the sorted source keys, duplicates allowed; sruns / n_su: pcc_unique_rows over
        them; svalues: a uint8 or uint16 [n_s, c] device tensor in the order of skeys; row_st int32 [n_s]: nn_frames'
        rows of skeys among the target's distinct keys; row_ts int32 [n_t]: its rows of those keys among the distinct
        source keys.  Returns (out, count): out [n_t, c] of the values' dtype (or `out`, a device tensor of at least
        n_t c values of it, written in place), count an int32 [n_t] device tensor holding uint32 values, None unless
        wanted.  Does not synchronise."""
        n_s, n_t = int(skeys.shape[0]), int(row_ts.shape[0])
        if svalues.dtype not in (torch.uint8, torch.uint16) or svalues.dim() != 2 or svalues.shape[0] != n_s or \
                row_st.shape[0] != n_s or (out is not None and (out.dtype != svalues.dtype or out.numel() < n_t * svalues.shape[1])):
            raise ValueError(f"attr_transfer_frames: values {tuple(svalues.shape)} {svalues.dtype} for {n_s} source rows")
        c = int(svalues.shape[1])
        if out is None:
            out = self.empty((n_t, c), svalues.dtype)
        count = self.empty((n_t,), torch.int32) if want_count else None
        check(self.lib.pcc_attr_transfer_frames(self.ctx, _ptr(skeys), n_s, _ptr(sruns), int(n_su), _ptr(svalues), _ptr(row_st),
                                                _ptr(row_ts), n_t, svalues.element_size(), c, int(n_frames), _ptr(out), _ptr(count)),
              "pcc_attr_transfer_frames")
        return out, count

    def attr_stage_frames(self, sources, row_offsets, scale=1.0, bpv=1, channels=0, perm=None):
        """per-point attributes from where they lie into the layout a consumer reads (pcc_attr_stage_frames, the rule of
        include/pcc.h).  sources: per frame (src, kind, c, pitch) — src a 2-D device tensor (its data_ptr is the frame's
        first value; pitch in elements) or a C-contiguous host array of the kind's dtype, which goes up raw in the one
        pinned upload that carries the row offsets and the per-frame table; kind one of ATTR_SRC_KINDS' values.
        row_offsets: the n_frames + 1 row offsets of the call.  scale: s of the rule, read for float kinds; bpv: bytes
        per value of float sources (packed) or of every row (sorted).
        channels == 0, packed: -> (values, value_offsets, status): a uint8 device tensor with frame f tight at
        value_offsets[f] (16-aligned) in its own width, as attr_encode_frames takes them (None for a call without a
        row).  channels 2 or 4, sorted: perm, the sort's permutation of the call's rows -> (values, None, status), values
        [n, channels] uint8 / uint16.  status: an int32 [1] device tensor, bit 0 a non-finite value, bit 1 a perm entry
        outside the call; not read here.  Does not synchronise."""
        nf, n = len(sources), int(row_offsets[-1])
        rec = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("out", "<i8"), ("kind", "<i4"), ("c", "<i4")])
        table_at = 8 * (nf + 1)
        at = raw_at = (table_at + rec.itemsize * nf + 15) // 16 * 16
        raws = []      # (frame, offset in the upload, host array)
        for f, (src, _, _, _) in enumerate(sources):
            if not isinstance(src, torch.Tensor) and src.size:
                raws.append((f, at, src))
                at += (src.nbytes + 15) // 16 * 16
        host = torch.empty(at, dtype=torch.uint8, pin_memory=True)
        h = host.numpy()
        h[table_at + rec.itemsize * nf:raw_at] = 0
        h[:table_at].view(np.int64)[:] = row_offsets
        table = h[table_at:table_at + rec.itemsize * nf].view(rec)
        dev = self.empty((at,), torch.uint8)      # before the table is written: the raw rows' addresses lie in it
        out_at = 0
        for f, (src, kind, c, pitch) in enumerate(sources):
            rows = int(row_offsets[f + 1] - row_offsets[f])
            own = (1, 2, bpv, bpv)[kind]
            table[f] = (src.data_ptr() if isinstance(src, torch.Tensor) and rows else 0, pitch, out_at, kind, c)
            out_at += (rows * c * own + 15) // 16 * 16
        for f, o, a in raws:
            h[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
            table["src"][f] = dev.data_ptr() + o
        dev.copy_(host, non_blocking=True)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        if channels:
            out = self.empty((n, channels), torch.uint8 if bpv == 1 else torch.uint16)
            nbytes = n * channels * bpv
        else:
            out = self.empty((max(out_at, 16),), torch.uint8) if n else None
            nbytes = out_at if n else 0
        check(self.lib.pcc_attr_stage_frames(self.ctx, C.c_void_p(host.data_ptr() + table_at), C.c_void_p(dev.data_ptr() + table_at),
                                             C.c_void_p(host.data_ptr()), C.c_void_p(dev.data_ptr()), nf, float(scale), int(bpv),
                                             int(channels), _ptr(perm), _ptr(out), nbytes, _ptr(status)), "pcc_attr_stage_frames")
        return out, None if channels else table["out"].tolist(), status

    def knn_frames(self, keys, n_frames, k, want_rows=False, want_dist=False, want_cov=False, want_normals=True,
                   viewpoint=None):
        """the k nearest neighbours of every point of a frame among the frame's own points, their scatter matrix and
        the surface normal (pcc_knn_frames, the rules of include/pcc.h).  keys: sorted distinct Morton keys on the
        device.  Returns (rows int32 [n, k], sqdist int64 [n, k] holding uint64 values, cov int64 [n, 6], normals
        float32 [n, 3]) as device tensors, None where not wanted.  viewpoint: three ints, or None.  Synchronises once,
        in front of the search (the checks of the keys); the results are on this runtime's stream."""
        n, k = int(keys.shape[0]), int(k)
        rows = self.empty((n, k), torch.int32) if want_rows else None
        sqdist = self.empty((n, k), torch.int64) if want_dist else None
        cov = self.empty((n, 6), torch.int64) if want_cov else None
        normals = self.empty((n, 3), torch.float32) if want_normals else None
        vp = None if viewpoint is None else (C.c_int * 3)(*[int(v) for v in viewpoint])
        check(self.lib.pcc_knn_frames(self.ctx, _ptr(keys), n, int(n_frames), k, _ptr(rows), _ptr(sqdist), _ptr(cov),
                                      _ptr(normals), vp), "pcc_knn_frames")
        return rows, sqdist, cov, normals

    # ------------------------------------------------------------ outlier removal (the rules of include/pcc.h)
    OUTLIER_KEEP_ALL = (1 << 64) - 1      # the threshold of a frame with fewer than 2 points

    @staticmethod
    def outlier_ratio(std_ratio):
        """R = rint(256 std_ratio) of the statistical rule, std_ratio in 0 .. 255"""
        return int(np.rint(256.0 * float(std_ratio)))

    @staticmethod
    def outlier_threshold(n, s1, s2, ratio):
        """T of the statistical rule in Python integers: the largest t with n t <= S1 or
        65536 (n - 1) (n t - S1)^2 <= R^2 n (n S2 - S1^2); n < 2 keeps everything.  Host only."""
        n, s1, s2, ratio = int(n), int(s1), int(s2), int(ratio)
        if n < 2:
            return Runtime.OUTLIER_KEEP_ALL
        return (s1 + math.isqrt(ratio * ratio * n * (n * s2 - s1 * s1) // (65536 * (n - 1)))) // n

    def outlier_scores_frames(self, keys, n_frames, k):
        """the statistical rule's scores (pcc_outlier_scores_frames).  keys: sorted distinct Morton keys on the device.
        Returns (scores, sums): scores an int64 [n] device tensor holding the uint64 q_i, sums a list of (S1, S2, n) per
        frame as Python ints, S2 joined from its two halves.  Synchronises."""
        n = int(keys.shape[0])
        scores = self.empty((n,), torch.int64)
        sums = self.empty((int(n_frames), 4), torch.int64)
        check(self.lib.pcc_outlier_scores_frames(self.ctx, _ptr(keys), n, int(n_frames), int(k), _ptr(scores), _ptr(sums)),
              "pcc_outlier_scores_frames")
        return scores, [(s1, lo + (hi << 32), cnt) for s1, lo, hi, cnt in self._u64_rows(sums)]

    def outlier_mask_frames(self, keys, n_frames, scores, thresholds):
        """keep = q <= T[frame] (pcc_outlier_mask_frames).  thresholds: n_frames Python ints below 2^64.  Returns (keep
        uint8 [n], kept int64 [n_frames]) as device tensors.  Synchronises once, in front of the kernel (the checks of
        the keys); the results are on this runtime's stream."""
        n = int(keys.shape[0])
        host = torch.empty(int(n_frames), dtype=torch.int64, pin_memory=True)
        host.numpy().view(np.uint64)[:] = np.array([int(t) for t in thresholds], dtype=np.uint64)
        keep = self.empty((n,), torch.uint8)
        kept = self.empty((int(n_frames),), torch.int64)
        check(self.lib.pcc_outlier_mask_frames(self.ctx, _ptr(keys), n, int(n_frames), _ptr(scores), _ptr(self.to_device(host)),
                                               _ptr(keep), _ptr(kept)), "pcc_outlier_mask_frames")
        return keep, kept

    def outlier_radius_frames(self, keys, n_frames, min_neighbours, radius2):
        """the radius rule (pcc_outlier_radius_frames).  Returns (keep uint8 [n], counts int64 [n_frames, 2]: points and
        kept points per frame) as device tensors.  Synchronises once, in front of the search."""
        n = int(keys.shape[0])
        keep = self.empty((n,), torch.uint8)
        counts = self.empty((int(n_frames), 2), torch.int64)
        check(self.lib.pcc_outlier_radius_frames(self.ctx, _ptr(keys), n, int(n_frames), int(min_neighbours),
                                                 min(int(radius2), Runtime.OUTLIER_KEEP_ALL), _ptr(keep), _ptr(counts)),
              "pcc_outlier_radius_frames")
        return keep, counts

    def outlier_compact_rows(self, index, keep, offsets_ptr, n_frames):
        """verdicts on distinct points -> the input rows of a call (pcc_outlier_compact_rows).  index: rows_index' result
        with no frame's rows taken off; keep: uint8 per distinct point; offsets_ptr: the input rows' frame offsets on the
        device.  Returns (mask uint8 [n], kept_rows int32 [n], kept_offsets int64 [n_frames + 1]) as device tensors:
        kept_rows holds, for the kept rows in input order, the row's place inside its frame.  Does not synchronise."""
        n = int(index.shape[0])
        mask = self.empty((n,), torch.uint8)
        kept_rows = self.empty((n,), torch.int32)
        kept_offsets = self.empty((int(n_frames) + 1,), torch.int64)
        check(self.lib.pcc_outlier_compact_rows(self.ctx, _ptr(index), n, _ptr(keep), int(keep.shape[0]), C.c_void_p(offsets_ptr),
                                                int(n_frames), _ptr(mask), _ptr(kept_rows), _ptr(kept_offsets)),
              "pcc_outlier_compact_rows")
        return mask, kept_rows, kept_offsets

    def take_rows(self, src, rows):
        """the rows `rows` (an int32 device tensor holding uint32 indices) of the 2-D device tensor src, whose rows are
        contiguous and may lie a pitch apart: pcc_gather_rows for tight rows of a multiple of 4 bytes, else
        pcc_gather_rows_pitched"""
        n, c = int(rows.shape[0]), int(src.shape[1])
        row_bytes = c * src.element_size()
        pitch = (int(src.stride(0)) if src.shape[0] > 1 else c) * src.element_size()
        dst = self.empty((n, c), src.dtype)
        if n == 0:
            return dst
        if pitch == row_bytes and row_bytes % 4 == 0:
            check(self.lib.pcc_gather_rows(self.ctx, _ptr(src), _ptr(rows), n, row_bytes, _ptr(dst)), "pcc_gather_rows")
        else:
            check(self.lib.pcc_gather_rows_pitched(self.ctx, C.c_void_p(src.data_ptr()), int(src.shape[0]), pitch, _ptr(rows), n, row_bytes,
                                                   _ptr(dst)), "pcc_gather_rows_pitched")
        return dst

    @staticmethod
    def outlier_replay_host(keys, n_frames, k=3, min_neighbours=1, radius2=0, thresholds=None):
        """both rules on the host (pcc_outlier_replay_host: the kernels' functions compiled for the host; no GPU
        needed, not a product path).  keys: a uint64 numpy array, sorted and distinct.  Returns a dict: scores uint64
        [n], sums [(S1, S2, n)] per frame, nodes uint32 [n]; keep uint8 [n] where thresholds (n_frames Python ints) are
        given; keep_radius / nodes_radius under the bounded search, keep_unbounded / nodes_unbounded under the k-NN
        search itself."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = int(keys.shape[0])
        u64, u32, u8 = (lambda: np.zeros(n, np.uint64)), (lambda: np.zeros(n, np.uint32)), (lambda: np.zeros(n, np.uint8))
        out = {"scores": u64(), "nodes": u32(), "keep_radius": u8(), "nodes_radius": u32(), "keep_unbounded": u8(),
               "nodes_unbounded": u32()}
        sums = np.zeros((int(n_frames), 4), np.uint64)
        th = None if thresholds is None else np.array([int(t) for t in thresholds], dtype=np.uint64)
        if th is not None:
            out["keep"] = u8()
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        check(_abi.lib().pcc_outlier_replay_host(ptr(keys), n, int(n_frames), int(k), int(min_neighbours),
                                                 min(int(radius2), Runtime.OUTLIER_KEEP_ALL), ptr(th), ptr(out["scores"]),
                                                 ptr(sums), ptr(out.get("keep")), ptr(out["nodes"]), ptr(out["keep_radius"]),
                                                 ptr(out["nodes_radius"]), ptr(out["keep_unbounded"]),
                                                 ptr(out["nodes_unbounded"])), "pcc_outlier_replay_host")
        out["sums"] = [(s1, lo + (hi << 32), cnt) for s1, lo, hi, cnt in sums.tolist()]
        return out

    # ------------------------------------------------------------ DBSCAN clusters (the rule of include/pcc.h)
    def cluster_frames(self, keys, n_frames, min_neighbours, radius2, min_points, want_sizes=True):
        """the clusters of every frame (pcc_cluster_frames).  keys: sorted distinct Morton keys on the device.  Returns
        (labels int32 [n], sizes int32 [n] holding uint32 values: frame f's sizes in label order from the frame's first
        row on, None unless wanted; counts int64 [n_frames, 4]: points, core points, clusters, noise points) as device
        tensors.  Synchronises once, in front of the kernels (the checks of the keys); the results are on this
        runtime's stream."""
        n = int(keys.shape[0])
        labels = self.empty((n,), torch.int32)
        sizes = self.empty((n,), torch.int32) if want_sizes else None
        counts = self.empty((int(n_frames), 4), torch.int64)
        check(self.lib.pcc_cluster_frames(self.ctx, _ptr(keys), n, int(n_frames), int(min_neighbours), int(radius2), int(min_points),
                                          _ptr(labels), _ptr(sizes), _ptr(counts)), "pcc_cluster_frames")
        return labels, sizes, counts

    @staticmethod
    def cluster_replay_host(keys, n_frames, min_neighbours=0, radius2=0, min_points=1, reversed_order=False):
        """the clustering rule on the host (pcc_cluster_replay_host: the kernels' functions compiled for the host; no
        GPU needed, not a product path).  keys: a uint64 numpy array, sorted and distinct.  Returns a dict: labels int32
        [n], sizes uint32 [n], counts [[points, core, clusters, noise]] per frame as Python ints, core uint8 [n], root
        int32 [n] (rows of the call, -1 without a component), nodes uint32 [n].  reversed_order: the unions of every
        frame issued from its last row to its first (pcc_cluster_replay_host_reversed)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = int(keys.shape[0])
        out = {"labels": np.zeros(n, np.int32), "sizes": np.zeros(n, np.uint32), "core": np.zeros(n, np.uint8),
               "root": np.zeros(n, np.int32), "nodes": np.zeros(n, np.uint32)}
        counts = np.zeros((max(int(n_frames), 0), 4), np.uint64)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        name = "pcc_cluster_replay_host_reversed" if reversed_order else "pcc_cluster_replay_host"
        check(getattr(_abi.lib(), name)(ptr(keys), n, int(n_frames), int(min_neighbours), int(radius2), int(min_points),
                                        ptr(out["labels"]), ptr(out["sizes"]), ptr(counts), ptr(out["core"]), ptr(out["root"]),
                                        ptr(out["nodes"])), name)
        out["counts"] = counts.tolist()
        return out

    def nn_d2_frames(self, qkeys, row, rkeys, normals, n_frames, normal_row=None, want_proj=False):
        """the D2 (point-to-plane) side of a pairing (pcc_nn_d2_frames): row, nn_frames' rows of qkeys among rkeys;
        normals a float32 [m, 3] device tensor; normal_row an int32 [n_q] device tensor, the row of normals to use for
        query i (every entry below m), or None: row i, and then m == n_q.  Returns (proj, sums): proj a float64 [n_q]
        device tensor (None unless want_proj), sums a list of n_frames floats.  Synchronises."""
        n_q = int(qkeys.shape[0])
        if normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[1] != 3 or row.shape[0] != n_q or \
                (normal_row is None and normals.shape[0] != n_q) or (normal_row is not None and normal_row.shape[0] != n_q):
            raise ValueError(f"nn_d2_frames: normals {tuple(normals.shape)} {normals.dtype} for {n_q} queries")
        proj = self.empty((n_q,), torch.float64) if want_proj else None
        sums = self.empty((n_frames,), torch.float64)
        check(self.lib.pcc_nn_d2_frames(self.ctx, _ptr(qkeys), _ptr(row), n_q, _ptr(rkeys), int(rkeys.shape[0]), _ptr(normals),
                                        _ptr(normal_row), int(n_frames), _ptr(proj), _ptr(sums)), "pcc_nn_d2_frames")
        self.sync()
        return proj, sums.cpu().tolist()

    def _u64_rows(self, t):
        """an int64 device tensor holding uint64 values, written on this runtime's stream -> nested lists of Python ints"""
        self.sync()
        return t.cpu().numpy().view(np.uint64).tolist()

    def linear_keys(self, coords):
        n = coords.shape[0]
        keys = self.empty((n,), torch.int64)
        check(self.lib.pcc_linear_keys(self.ctx, _ptr(coords), n, _ptr(keys)), "pcc_linear_keys")
        return keys

    def sort_pairs(self, keys, signed=False):
        """sorts `keys` in place, returns the permutation (int32 tensor holding uint32 indices)"""
        n = keys.shape[0]
        perm = self.empty((n,), torch.int32)
        check(self.lib.pcc_sort_pairs(self.ctx, _ptr(keys), _ptr(perm), n, 1 if signed else 0), "pcc_sort_pairs")
        return perm

    def sort_coords(self, coords):
        n = coords.shape[0]
        perm = self.empty((n,), torch.int32)
        check(self.lib.pcc_sort_coords(self.ctx, _ptr(coords), n, _ptr(perm)), "pcc_sort_coords")
        return perm

    def gather_rows(self, src, perm):
        n = perm.shape[0]
        row_elems = 1
        for d in src.shape[1:]:
            row_elems *= int(d)
        row_bytes = src.element_size() * row_elems
        dst = self.empty((n,) + tuple(src.shape[1:]), src.dtype)
        check(self.lib.pcc_gather_rows(self.ctx, _ptr(src), _ptr(perm), n, row_bytes, _ptr(dst)), "pcc_gather_rows")
        return dst

    def check_unique(self, sorted_keys):
        dup = C.c_int(0)
        check(self.lib.pcc_check_unique(self.ctx, _ptr(sorted_keys), sorted_keys.shape[0], C.byref(dup)),
              "pcc_check_unique")
        return dup.value == 0

    def batch_offsets(self, keys, n_batch):
        out = (C.c_int64 * (n_batch + 1))()
        check(self.lib.pcc_batch_offsets(self.ctx, _ptr(keys), keys.shape[0], n_batch, out), "pcc_batch_offsets")
        return [int(v) for v in out]

    # ------------------------------------------------------------ pyramid / maps
    def down_coords(self, keys, child_shift, m_known=None):
        """m_known: the parent count from level_counts — then the call does not synchronise"""
        n = keys.shape[0]
        pkeys = self.empty((n,), torch.int64)
        nbr8 = self.empty((8 * n,), torch.int32)
        parent_of = self.empty((n,), torch.int32)
        if m_known is None:
            m = C.c_int64(0)
            check(self.lib.pcc_down_coords(self.ctx, _ptr(keys), n, child_shift, _ptr(pkeys), _ptr(nbr8), n,
                                           _ptr(parent_of), C.byref(m)), "pcc_down_coords")
            m = m.value
        else:
            m = int(m_known)
            check(self.lib.pcc_down_coords_known(self.ctx, _ptr(keys), n, child_shift, _ptr(pkeys), _ptr(nbr8), n,
                                                 _ptr(parent_of), m), "pcc_down_coords_known")
        return pkeys[:m], nbr8[:8 * m].view(8, m), parent_of

    def level_counts(self, keys, child_shift, levels):
        """([rows of the `levels` successive parent sets of a sorted key set], duplicate-rows flag): one pass"""
        cnt = (C.c_int64 * levels)()
        dup = C.c_int(0)
        check(self.lib.pcc_level_counts(self.ctx, _ptr(keys), keys.shape[0], child_shift, levels, cnt, C.byref(dup)),
              "pcc_level_counts")
        return [int(v) for v in cnt], bool(dup.value)

    def derive_map_up(self, nbr_parent, n_parents, parent_rows=None, remap=None):
        nbr = self.empty((27, 8 * n_parents), torch.int32)
        check(self.lib.pcc_derive_map_up(self.ctx, _ptr(nbr_parent), nbr_parent.stride(0),
                                         _ptr(parent_rows) if parent_rows is not None else C.c_void_p(0),
                                         _ptr(remap) if remap is not None else C.c_void_p(0), n_parents,
                                         _ptr(nbr)), "pcc_derive_map_up")
        return nbr

    def subset_map_up(self, nbr_parent, keep, remap):
        """rule book [27, n_keep] of the rows `keep` of the 8 n generative children of a level with book nbr_parent"""
        n_keep = keep.shape[0]
        nbr = self.empty((27, n_keep), torch.int32)
        check(self.lib.pcc_subset_map_up(self.ctx, _ptr(nbr_parent), nbr_parent.stride(0), _ptr(keep), _ptr(remap),
                                         n_keep, _ptr(nbr)), "pcc_subset_map_up")
        return nbr

    def gather_map_columns(self, nbr, rows):
        """(rule book [K, m] of the subset rows `rows` (int32, -1 = absent) of a level with book nbr [K, n],
        self [m] = j where rows[j] >= 0 else -1)"""
        k_vol, m = nbr.shape[0], rows.shape[0]
        out = self.empty((k_vol, m), torch.int32)
        me = self.empty((m,), torch.int32)
        check(self.lib.pcc_gather_map_columns(self.ctx, _ptr(nbr), k_vol, nbr.stride(0), _ptr(rows), m, _ptr(out),
                                              _ptr(me)), "pcc_gather_map_columns")
        return out, me

    def derive_map_down(self, nbr_parent, nbr8, parent_of, keys, child_shift):
        n = keys.shape[0]
        nbr = self.empty((27, n), torch.int32)
        check(self.lib.pcc_derive_map_down(self.ctx, _ptr(nbr_parent), nbr_parent.shape[1], _ptr(nbr8),
                                           _ptr(parent_of), _ptr(keys), n, child_shift, _ptr(nbr)),
              "pcc_derive_map_down")
        return nbr

    def inverse_rows(self, rows, n):
        remap = self.empty((n,), torch.int32)
        check(self.lib.pcc_inverse_rows(self.ctx, _ptr(rows), rows.shape[0], n, _ptr(remap)), "pcc_inverse_rows")
        return remap

    def up_coords(self, keys, child_shift):
        n = keys.shape[0]
        ckeys = self.empty((8 * n,), torch.int64)
        check(self.lib.pcc_up_coords(self.ctx, _ptr(keys), n, child_shift, _ptr(ckeys)), "pcc_up_coords")
        return ckeys

    def up_coords_rows(self, keys, child_shift, rows):
        """Keys of the listed generative children (rows[i] = 8 p + o) without the 8 n keys being formed."""
        m = rows.shape[0]
        ckeys = self.empty((m,), torch.int64)
        check(self.lib.pcc_up_coords_rows(self.ctx, _ptr(keys), keys.shape[0], child_shift, _ptr(rows), m, _ptr(ckeys)),
              "pcc_up_coords_rows")
        return ckeys

    def build_map(self, keys, stride):
        n = keys.shape[0]
        nbr = self.empty((27, n), torch.int32)
        check(self.lib.pcc_build_map(self.ctx, _ptr(keys), n, stride, _ptr(nbr)), "pcc_build_map")
        return nbr

    def lookup(self, keys, qkeys):
        m = qkeys.shape[0]
        rows = self.empty((m,), torch.int32)
        check(self.lib.pcc_lookup(self.ctx, _ptr(keys), keys.shape[0], _ptr(qkeys), m, _ptr(rows)), "pcc_lookup")
        return rows

    def gather_rows_or_zero(self, src, rows):
        m, c = rows.shape[0], src.shape[1]
        dst = self.empty((m, c), torch.float32)
        check(self.lib.pcc_gather_rows_or_zero(self.ctx, _ptr(src), _ptr(rows), m, c, _ptr(dst)),
              "pcc_gather_rows_or_zero")
        return dst

    # ------------------------------------------------------------ layers
    def sparse_conv(self, x, nbr, w, b, relu):
        k_vol, n_out = nbr.shape
        cin, cout = w.shape[1], w.shape[2]
        assert x.shape[1] == cin and w.shape[0] == k_vol, (x.shape, w.shape, nbr.shape)
        out = self.empty((n_out, cout), torch.float32)
        check(self.lib.pcc_sparse_conv(self.ctx, _ptr(x), x.shape[0], _ptr(nbr), k_vol, nbr.stride(0), n_out,
                                       _ptr(w), _ptr(b), cin, cout, 1 if relu else 0, _ptr(out)),
              "pcc_sparse_conv")
        return out

    def sparse_conv_head(self, x, nbr, w, b, relu, head_w, head_b):
        """conv layer + fused 1x1 head (cout -> 1): returns (features [n,cout], logits [n])"""
        k_vol, n_out = nbr.shape
        cin, cout = w.shape[1], w.shape[2]
        assert x.shape[1] == cin and w.shape[0] == k_vol and head_w.numel() == cout
        out = self.empty((n_out, cout), torch.float32)
        logits = self.empty((n_out,), torch.float32)
        check(self.lib.pcc_sparse_conv_head(self.ctx, _ptr(x), x.shape[0], _ptr(nbr), k_vol, nbr.stride(0), n_out,
                                            _ptr(w), _ptr(b), cin, cout, 1 if relu else 0, _ptr(out),
                                            _ptr(head_w), _ptr(head_b), _ptr(logits)), "pcc_sparse_conv_head")
        return out, logits

    def sparse_conv_head_up(self, x, nbr_parent, w, b, relu, head_w, head_b):
        """sparse_conv_head on the 8 n generative children of a level, given THAT level's rule book [27, n]:
        the child rule book is formed inside the kernel (same bits as derive_map_up + sparse_conv_head)"""
        n_parents = nbr_parent.shape[1]
        assert x.shape == (8 * n_parents, 32) and w.shape == (27, 32, 32) and head_w.numel() == 32
        out = self.empty((8 * n_parents, 32), torch.float32)
        logits = self.empty((8 * n_parents,), torch.float32)
        check(self.lib.pcc_sparse_conv_head_up(self.ctx, _ptr(x), n_parents, _ptr(nbr_parent), nbr_parent.stride(0),
                                               _ptr(w), _ptr(b), 1 if relu else 0, _ptr(out), _ptr(head_w),
                                               _ptr(head_b), _ptr(logits)), "pcc_sparse_conv_head_up")
        return out, logits

    def conv_prepare(self, w):
        """register the weights [k, 32, 32|64] of a layer: re-arranged once, found by pointer afterwards (pcc_conv_prepare)"""
        check(self.lib.pcc_conv_prepare(self.ctx, _ptr(w), w.shape[0], w.shape[1], w.shape[2]), "pcc_conv_prepare")

    def conv_forget(self, w):
        check(self.lib.pcc_conv_forget(self.ctx, _ptr(w)), "pcc_conv_forget")

    def convT_gen(self, x, w, b, relu):
        n, cin, cout = x.shape[0], w.shape[1], w.shape[2]
        assert x.shape[1] == cin and w.shape[0] == 8
        out = self.empty((8 * n, cout), torch.float32)
        check(self.lib.pcc_convT_gen(self.ctx, _ptr(x), n, _ptr(w), _ptr(b), cin, cout, 1 if relu else 0,
                                     _ptr(out)), "pcc_convT_gen")
        return out

    def linear(self, x, w, b, relu):
        n, cin, cout = x.shape[0], w.shape[0], w.shape[1]
        assert x.shape[1] == cin
        out = self.empty((n, cout), torch.float32)
        check(self.lib.pcc_linear(self.ctx, _ptr(x), n, _ptr(w), _ptr(b), cin, cout, 1 if relu else 0, _ptr(out)),
              "pcc_linear")
        return out

    def convT_gen_gather(self, x, rows, w, b, relu):
        """convT_gen (32 -> 32) whose parent p is row rows[p] of x: [8 len(rows), 32]"""
        n = rows.shape[0]
        assert x.shape[1] == 32 and w.shape == (8, 32, 32)
        out = self.empty((8 * n, 32), torch.float32)
        check(self.lib.pcc_convT_gen_gather(self.ctx, _ptr(x), _ptr(rows), n, _ptr(w), _ptr(b), 1 if relu else 0,
                                            _ptr(out)), "pcc_convT_gen_gather")
        return out

    def linear_gather(self, x, rows, w, b, relu):
        """linear (cin 32, cout <= 8) on the rows `rows` (int32) of x: [len(rows), cout]"""
        n, cout = rows.shape[0], w.shape[1]
        assert x.shape[1] == 32 and w.shape[0] == 32
        out = self.empty((n, cout), torch.float32)
        check(self.lib.pcc_linear_gather(self.ctx, _ptr(x), _ptr(rows), n, _ptr(w), _ptr(b), cout, 1 if relu else 0,
                                         _ptr(out)), "pcc_linear_gather")
        return out

    def topk_prune(self, logits, offsets, k, with_map=False):
        """Kept rows (ascending); with_map: also remap [n] = position of a row among the kept ones, or -1."""
        n, nb = logits.shape[0], len(k)
        keep = self.empty((n,), torch.int32)
        offs = (C.c_int64 * (nb + 1))(*offsets)
        ks = (C.c_int64 * nb)(*k)
        nk = C.c_int64(0)
        if with_map:
            remap = self.empty((n,), torch.int32)
            check(self.lib.pcc_topk_prune_map(self.ctx, _ptr(logits), n, nb, offs, ks, _ptr(keep), C.byref(nk), _ptr(remap)),
                  "pcc_topk_prune_map")
            return keep[:nk.value], remap
        check(self.lib.pcc_topk_prune(self.ctx, _ptr(logits), n, nb, offs, ks, _ptr(keep), C.byref(nk)),
              "pcc_topk_prune")
        return keep[:nk.value]

    # ------------------------------------------------------------ entropy (device part)
    def factorized_quant(self, z, med):
        n, c = z.shape
        sym = self.empty((c, n), torch.int32)
        zhat = self.empty((n, c), torch.float32)
        check(self.lib.pcc_factorized_quant(self.ctx, _ptr(z), n, c, _ptr(med), _ptr(sym), _ptr(zhat)),
              "pcc_factorized_quant")
        return sym, zhat

    def factorized_dequant(self, sym, med):
        c, n = sym.shape
        zhat = self.empty((n, c), torch.float32)
        check(self.lib.pcc_factorized_dequant(self.ctx, _ptr(sym), n, c, _ptr(med), _ptr(zhat)),
              "pcc_factorized_dequant")
        return zhat

    def gaussian_quant(self, y, params, scale, table):
        n, c = y.shape
        q = scale.shape[0]
        sym = self.empty((q, c, n), torch.int32)
        idx = self.empty((q, c, n), torch.int32)
        check(self.lib.pcc_gaussian_quant(self.ctx, _ptr(y), _ptr(params), n, c, _ptr(scale), q, _ptr(table),
                                          table.shape[0], _ptr(sym), _ptr(idx)), "pcc_gaussian_quant")
        return sym, idx

    def build_indexes(self, scales, table):
        """element-wise GaussianConditional.build_indexes on a tensor of any shape"""
        scales = scales.contiguous()
        idx = self.empty(tuple(scales.shape), torch.int32)
        check(self.lib.pcc_build_indexes(self.ctx, _ptr(scales), scales.numel(), _ptr(table), table.shape[0],
                                         _ptr(idx)), "pcc_build_indexes")
        return idx

    def quantize_symbols(self, x, means=None):
        """element-wise round(x - means) -> int32 (EntropyModel.quantize(..., "symbols", means))"""
        x = x.contiguous()
        means = means.contiguous() if means is not None else None
        sym = self.empty(tuple(x.shape), torch.int32)
        check(self.lib.pcc_quantize_symbols(self.ctx, _ptr(x), _ptr(means), x.numel(), _ptr(sym)),
              "pcc_quantize_symbols")
        return sym

    def gaussian_quant16(self, y, params, scale, table):
        """compact form: int16 symbols, uint8 indexes, overflow flag (device int32[1])"""
        n, c = y.shape
        q = scale.shape[0]
        sym = self.empty((q, c, n), torch.int16)
        idx = self.empty((q, c, n), torch.uint8)
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(self.lib.pcc_gaussian_quant16(self.ctx, _ptr(y), _ptr(params), n, c, _ptr(scale), q, _ptr(table),
                                            table.shape[0], _ptr(sym), _ptr(idx), _ptr(flag)),
              "pcc_gaussian_quant16")
        return sym, idx, flag

    def gaussian_quant_dev(self, y, params, scale, table):
        """int32 symbols, uint8 indexes — the element types the GPU coder reads (pcc_gaussian_quant_dev)"""
        n, c = y.shape
        q = scale.shape[0]
        sym = self.empty((q, c, n), torch.int32)
        idx = self.empty((q, c, n), torch.uint8)
        check(self.lib.pcc_gaussian_quant_dev(self.ctx, _ptr(y), _ptr(params), n, c, _ptr(scale), q, _ptr(table),
                                              table.shape[0], _ptr(sym), _ptr(idx)), "pcc_gaussian_quant_dev")
        return sym, idx

    def gaussian_indexes8(self, params, scale, table):
        n, c = params.shape[0], params.shape[1] // 2
        idx = self.empty((c, n), torch.uint8)
        check(self.lib.pcc_gaussian_indexes8(self.ctx, _ptr(params), n, c, _ptr(scale), _ptr(table),
                                             table.shape[0], _ptr(idx)), "pcc_gaussian_indexes8")
        return idx

    # ------------------------------------------------------------ pinned staging
    def pinned(self, key, nbytes):
        """a cached page-locked host buffer of at least nbytes (uint8 tensor)"""
        pool = self.__dict__.setdefault("_pin", {})
        buf = pool.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 4096), dtype=torch.uint8, pin_memory=True)
            pool[key] = buf
        return buf

    def to_host_async(self, t, key):
        """device tensor -> numpy view of a pinned buffer; valid after the next sync()"""
        nbytes = t.numel() * t.element_size()
        buf = self.pinned(key, nbytes)[:nbytes].view(t.dtype).view(t.shape)
        buf.copy_(t, non_blocking=True)
        return buf.numpy()

    def from_pinned_async(self, host_tensor):
        """pinned host tensor -> new device tensor (async on this runtime's stream)"""
        return host_tensor.to(self.device, non_blocking=True)

    def gaussian_indexes(self, params, scale, table):
        n, c = params.shape[0], params.shape[1] // 2
        idx = self.empty((c, n), torch.int32)
        check(self.lib.pcc_gaussian_indexes(self.ctx, _ptr(params), n, c, _ptr(scale), _ptr(table),
                                            table.shape[0], _ptr(idx)), "pcc_gaussian_indexes")
        return idx

    def gaussian_dequant(self, sym, params, scale, bound, off_a, off_b):
        c, n = sym.shape
        yhat = self.empty((n, c), torch.float32)
        check(self.lib.pcc_gaussian_dequant(self.ctx, _ptr(sym), _ptr(params), n, c, _ptr(scale), bound, off_a,
                                            off_b, _ptr(yhat)), "pcc_gaussian_dequant")
        return yhat

    # ------------------------------------------------------------ octree (device part)
    def octree_levels(self, keys, key_shift, depth):
        n = keys.shape[0]
        cap = n * depth
        occ = self.empty((cap,), torch.uint8)
        level_n = (C.c_int64 * depth)()
        check(self.lib.pcc_octree_levels(self.ctx, _ptr(keys), n, key_shift, depth, _ptr(occ), cap, level_n),
              "pcc_octree_levels")
        ln = [int(v) for v in level_n]
        return occ[:sum(ln)], ln

    def octree_encode(self, keys, key_shift, version=0):
        """geometry blob of one frame's Morton-sorted keys (pcc_octree_encode_version): version 0 = the library's rule —
        blob version 2 (occupancy coder on the GPU, csrc/octree2.hip) above PCC_OCTREE_V2_MIN_LEAVES leaves, version 1
        (serial host coder) below"""
        n = keys.shape[0]
        cap = 4096 + 17 * max(n, 1)          # one byte per node at most, plus header and chunk table
        out = np.empty(cap, dtype=np.uint8)
        length = C.c_int64(0)
        check(self.lib.pcc_octree_encode_version(self.ctx, _ptr(keys), n, key_shift, version, _np_ptr(out), cap,
                                                 C.byref(length)), "pcc_octree_encode")
        return out[:length.value].tobytes()

    def octree_decode(self, blob):
        """blob (either version) -> int32 [n,3] host array, Morton order (pcc_octree_decode_ctx: version 2 is decoded
        by the GPU)"""
        buf = np.frombuffer(blob, dtype=np.uint8)
        n = C.c_int64(0)
        check(self.lib.pcc_octree_decode_ctx(self.ctx, _np_ptr(buf), buf.shape[0], None, 0, C.byref(n)), "pcc_octree_decode_ctx")
        pts = np.empty((n.value, 3), dtype=np.int32)
        if n.value:
            check(self.lib.pcc_octree_decode_ctx(self.ctx, _np_ptr(buf), buf.shape[0], _np_ptr(pts), n.value, C.byref(n)),
                  "pcc_octree_decode_ctx")
        return pts

    def octree_encode_frames(self, keys, n_frames, key_shift=0):
        """version-2 blobs of n_frames frames at once (pcc_octree_encode_frames): `keys` Morton-sorted and distinct, the
        batch index of a key is its frame.  A list of n_frames bytes objects, blob f equal to octree_encode(frame f's
        keys, key_shift, version=2); a frame without keys gives the 24-byte empty blob."""
        n = keys.shape[0]
        cap = 4096 * n_frames + 17 * max(n, 1)
        out = np.empty(cap, dtype=np.uint8)
        offs = (C.c_int64 * (n_frames + 1))()
        check(self.lib.pcc_octree_encode_frames(self.ctx, _ptr(keys), n, n_frames, key_shift, _np_ptr(out), cap, offs),
              "pcc_octree_encode_frames")
        return [out[offs[f]:offs[f + 1]].tobytes() for f in range(n_frames)]

    @staticmethod
    def octree_lod_info(blob, lod):
        """(bytes, cells) of level of detail `lod` (0 .. 15) of a version-2 or version-4 blob (pcc_octree_lod_info, host
        only): the shortest prefix of the blob that decodes at that level, and the cells it gives.  `blob` may itself be
        a prefix that reaches the last needed chunk's length table."""
        buf = np.frombuffer(blob, dtype=np.uint8)
        nbytes, cells = C.c_int64(0), C.c_int64(0)
        check(_abi.lib().pcc_octree_lod_info(_np_ptr(buf) if buf.shape[0] else None, buf.shape[0], int(lod),
                                             C.byref(nbytes), C.byref(cells)), "pcc_octree_lod_info")
        return nbytes.value, cells.value

    def octree_decode_frames(self, blobs, device=False, lod=0, whole=False):
        """version-2 blobs -> one int32 [n_f, 3] array per blob, Morton order (pcc_octree_decode_frames_lod): numpy
        arrays, or views of one device tensor (device=True).  lod = k > 0: blobs or prefixes of them (octree_lod_info)
        -> the distinct cell indices points >> k of every frame, Morton order.  whole=True: (that list, the one array
        or tensor [total, 3] its entries are views of)"""
        nb = len(blobs)
        if nb == 0:
            return ([], None) if whole else []
        lod = int(lod)
        if lod == 0:      # today's call, by its own name
            name = "pcc_octree_decode_frames"
            call = lambda *a: self.lib.pcc_octree_decode_frames(self.ctx, ptrs, lens, nb, *a, offs)
        else:
            name = "pcc_octree_decode_frames_lod"
            call = lambda *a: self.lib.pcc_octree_decode_frames_lod(self.ctx, ptrs, lens, nb, lod, *a, offs)
        bufs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
        ptrs = (C.c_void_p * nb)(*[b.ctypes.data if b.shape[0] else None for b in bufs])
        lens = (C.c_int64 * nb)(*[b.shape[0] for b in bufs])
        offs = (C.c_int64 * (nb + 1))()
        pts = self._sized_output(call, name, offs, lambda total: (total, 3), torch.int32, device)
        views = [pts[offs[f]:offs[f + 1]] for f in range(nb)]
        return (views, pts) if whole else views

    def octree_encode_frames_inter(self, keys, n_frames, key_shift=0, intra_period=0, ref_first=False):
        """octree_encode_frames with inter-frame prediction (pcc_octree_encode_frames_inter; include/pcc.h has the
        rule): every frame but the intra ones — the coded frames g with g % intra_period == 0, or with intra_period 0
        the first frame of the keys alone — is a blob of version 4, coded against the frame in front of it.
        ref_first: frame 0 of the keys is only the reference of frame 1 and gets no blob: n_frames - 1 blobs."""
        n = keys.shape[0]
        cap = 8192 * n_frames + 17 * max(n, 1)
        out = np.empty(cap, dtype=np.uint8)
        offs = (C.c_int64 * (n_frames + 1))()
        check(self.lib.pcc_octree_encode_frames_inter(self.ctx, _ptr(keys), n, n_frames, key_shift, int(intra_period),
                                                      1 if ref_first else 0, _np_ptr(out), cap, offs),
              "pcc_octree_encode_frames_inter")
        return [out[offs[f]:offs[f + 1]].tobytes() for f in range(1 if ref_first else 0, n_frames)]

    def octree_decode_frames_ref(self, blobs, reference=None, device=False, whole=False):
        """blobs of versions 2 and 4 in any mix -> one int32 [n_f, 3] array per blob, as octree_decode_frames
        (pcc_octree_decode_frames_ref).  The reference of a version-4 blob is the frame decoded before it; for blob 0 it
        is `reference`, an int32 [n, 3] device tensor of distinct points in Morton order, as a decode returns them."""
        nb = len(blobs)
        if nb == 0:
            return ([], None) if whole else []
        bufs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
        ptrs = (C.c_void_p * nb)(*[b.ctypes.data if b.shape[0] else None for b in bufs])
        lens = (C.c_int64 * nb)(*[b.shape[0] for b in bufs])
        offs = (C.c_int64 * (nb + 1))()
        n_ref = 0 if reference is None else int(reference.shape[0])
        ref_ptr = _ptr(reference) if n_ref else None
        call = lambda *a: self.lib.pcc_octree_decode_frames_ref(self.ctx, ptrs, lens, nb, ref_ptr, n_ref, *a, offs)
        pts = self._sized_output(call, "pcc_octree_decode_frames_ref", offs, lambda total: (total, 3), torch.int32, device)
        views = [pts[offs[f]:offs[f + 1]] for f in range(nb)]
        return (views, pts) if whole else views

    def octree_encode_frames_inter_hist(self, keys, n_frames, key_shift=0, intra_period=0, n_ref_frames=0, history=1):
        """octree_encode_frames_inter with windows of up to `history` (1 .. 8) frames
        (pcc_octree_encode_frames_inter_hist; include/pcc.h has the rule): a predicted frame is coded against the union
        of the frames of its window, byte 3 of its blob holds their number - 1.  The first n_ref_frames (0 .. history)
        frames of the keys are only references and get no blob: n_frames - n_ref_frames blobs."""
        n = keys.shape[0]
        cap = 8192 * n_frames + 17 * max(n, 1)
        out = np.empty(cap, dtype=np.uint8)
        offs = (C.c_int64 * (n_frames + 1))()
        check(self.lib.pcc_octree_encode_frames_inter_hist(self.ctx, _ptr(keys), n, n_frames, key_shift, int(intra_period),
                                                           int(n_ref_frames), int(history), _np_ptr(out), cap, offs),
              "pcc_octree_encode_frames_inter_hist")
        return [out[offs[f]:offs[f + 1]].tobytes() for f in range(int(n_ref_frames), n_frames)]

    def octree_encode_frames_inter_best(self, keys, n_frames, key_shift=0, intra_period=0, n_ref_frames=0, history=1):
        """octree_encode_frames_inter_hist's arguments, every frame written as the shortest of its candidates
        (pcc_octree_encode_frames_inter_best; include/pcc.h has the rule): its version-2 blob and its version-4 blobs
        against the windows 1 .. what `history` gives it; of equal lengths version 2, then the smaller window.  A
        version-2 blob written by choice cuts no window behind it."""
        n = keys.shape[0]
        cap = 8192 * n_frames + 17 * max(n, 1)
        out = np.empty(cap, dtype=np.uint8)
        offs = (C.c_int64 * (n_frames + 1))()
        check(self.lib.pcc_octree_encode_frames_inter_best(self.ctx, _ptr(keys), n, n_frames, key_shift, int(intra_period),
                                                           int(n_ref_frames), int(history), _np_ptr(out), cap, offs),
              "pcc_octree_encode_frames_inter_best")
        return [out[offs[f]:offs[f + 1]].tobytes() for f in range(int(n_ref_frames), n_frames)]

    def octree_decode_frames_refs(self, blobs, references=(), device=False, whole=False):
        """octree_decode_frames_ref with up to 8 references, oldest first (pcc_octree_decode_frames_refs): each an int32
        [n, 3] device tensor of distinct points in Morton order.  A version-4 blob says in its byte 3 how many of the
        frames in front of it — the references, then the frames decoded in the call — its reference is the union of."""
        nb = len(blobs)
        if nb == 0:
            return ([], None) if whole else []
        bufs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
        ptrs = (C.c_void_p * nb)(*[b.ctypes.data if b.shape[0] else None for b in bufs])
        lens = (C.c_int64 * nb)(*[b.shape[0] for b in bufs])
        offs = (C.c_int64 * (nb + 1))()
        nr = len(references)
        ref_ptrs = (C.c_void_p * max(nr, 1))(*[_ptr(r) if r.shape[0] else None for r in references])
        ref_n = (C.c_int64 * max(nr, 1))(*[int(r.shape[0]) for r in references])
        call = lambda *a: self.lib.pcc_octree_decode_frames_refs(self.ctx, ptrs, lens, nb, ref_ptrs, ref_n, nr, *a, offs)
        pts = self._sized_output(call, "pcc_octree_decode_frames_refs", offs, lambda total: (total, 3), torch.int32, device)
        views = [pts[offs[f]:offs[f + 1]] for f in range(nb)]
        return (views, pts) if whole else views

    def octree_decode_frames_refs_lod(self, blobs, references=(), lod=0, device=False, whole=False):
        """octree_decode_frames_refs at a level of detail (pcc_octree_decode_frames_refs_lod): blobs of versions 2 and 4
        or prefixes of them (octree_lod_info) -> the cells points >> lod of every frame.  lod > 0: the references are
        CELLS at that lod, int32 [n, 3] device tensors, distinct and in Morton order, as this call returns them."""
        nb = len(blobs)
        if nb == 0:
            return ([], None) if whole else []
        bufs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
        ptrs = (C.c_void_p * nb)(*[b.ctypes.data if b.shape[0] else None for b in bufs])
        lens = (C.c_int64 * nb)(*[b.shape[0] for b in bufs])
        offs = (C.c_int64 * (nb + 1))()
        nr = len(references)
        ref_ptrs = (C.c_void_p * max(nr, 1))(*[_ptr(r) if r.shape[0] else None for r in references])
        ref_n = (C.c_int64 * max(nr, 1))(*[int(r.shape[0]) for r in references])
        call = lambda *a: self.lib.pcc_octree_decode_frames_refs_lod(self.ctx, ptrs, lens, nb, ref_ptrs, ref_n, nr, int(lod), *a, offs)
        pts = self._sized_output(call, "pcc_octree_decode_frames_refs_lod", offs, lambda total: (total, 3), torch.int32, device)
        views = [pts[offs[f]:offs[f + 1]] for f in range(nb)]
        return (views, pts) if whole else views

    def merge_keys(self, lists, key_shift=0):
        """the union of 1 .. 8 lists of Morton keys (pcc_merge_keys): int64 device tensors, each strictly increasing
        under (key & (2^48 - 1)) >> key_shift -> one int64 device tensor, strictly increasing under the same comparison;
        of equal keys the one of the first list that holds it is kept, bits from 48 up are carried along."""
        nl = len(lists)
        total = sum(int(k.shape[0]) for k in lists)
        out = torch.empty(max(total, 1), dtype=torch.int64, device=self.device)
        ptrs = (C.c_void_p * max(nl, 1))(*[_ptr(k) if k.shape[0] else None for k in lists])
        ns = (C.c_int64 * max(nl, 1))(*[int(k.shape[0]) for k in lists])
        count = C.c_int64(0)
        check(self.lib.pcc_merge_keys(self.ctx, ptrs, ns, nl, int(key_shift), _ptr(out), total, C.byref(count)), "pcc_merge_keys")
        return out[:count.value]

    def merge_keys_nested(self, lists, key_shift=0):
        """the nested unions of 1 .. 8 lists of Morton keys, NEWEST FIRST (pcc_merge_keys_nested): lists as merge_keys
        takes them -> [union 1, .., union len(lists)], union W that of lists[:W], int64 device tensors (views of one),
        formed in one pass; of equal keys the one of the first list that holds it is kept."""
        nl = len(lists)
        sizes = [int(k.shape[0]) for k in lists]
        rooms = list(np.cumsum(sizes)) if nl else []
        out = torch.empty(max(int(sum(rooms)), 1), dtype=torch.int64, device=self.device)
        ptrs = (C.c_void_p * max(nl, 1))(*[_ptr(k) if k.shape[0] else None for k in lists])
        ns = (C.c_int64 * max(nl, 1))(*sizes)
        counts = (C.c_int64 * max(nl, 1))()
        check(self.lib.pcc_merge_keys_nested(self.ctx, ptrs, ns, nl, int(key_shift), _ptr(out), int(sum(rooms)), counts),
              "pcc_merge_keys_nested")
        starts = [int(sum(rooms[:w])) for w in range(nl)]
        return [out[starts[w]:starts[w] + counts[w]] for w in range(nl)]

    @staticmethod
    def octree_inter_info(blob):
        """what the head of a geometry blob of version 2 or 4 says (pcc_octree_inter_info, host only; the blob whole, or
        for version 4 exactly a prefix that octree_lod_info names): {"version", "points", "predicted",
        "reference_points"}"""
        buf = np.frombuffer(blob, dtype=np.uint8)
        version, predicted = C.c_int(0), C.c_int(0)
        points, ref_points = C.c_int64(0), C.c_int64(0)
        check(_abi.lib().pcc_octree_inter_info(_np_ptr(buf) if buf.shape[0] else None, buf.shape[0], C.byref(version),
                                               C.byref(points), C.byref(predicted), C.byref(ref_points)), "pcc_octree_inter_info")
        return {"version": version.value, "points": points.value, "predicted": bool(predicted.value),
                "reference_points": ref_points.value}

    def _sized_output(self, call, name, offs, shape, dtype, device):
        """the two phases of a frame decoder's output: call(None, None, 0) for the sizes, which it leaves in `offs`; then
        shape(total) of `dtype` on the device, or pinned on the host, where the library copies straight into it (torch's
        host cache keeps the pages mapped); then call(device output, host output, total), only if there is any -> the
        tensor, or the numpy view of the pinned one"""
        check(call(None, None, 0), name)
        total = offs[len(offs) - 1]
        if device:
            out = self.empty(shape(total), dtype)
        else:
            out = torch.empty(shape(total), dtype=dtype, pin_memory=True).numpy()
        if total:
            check(call(_ptr(out), None, total) if device else call(None, _np_ptr(out), total), name)
        return out

    def attr_encode_frames(self, values, value_offsets, formats, row_offsets, points, perm, run_starts, n_unique,
                           version=1, keys=None, key_shift=0, n_kept=None, max_error=0, cross=None, qstep=0, colour=None,
                           scalable_to=None):
        """attribute blobs (csrc/attr.hip) of len(formats) frames at once (pcc_attr_encode_frames): `values` a
        device uint8 tensor with frame f's [rows_f, c_f] values at byte value_offsets[f], formats[f] = bytes per value |
        c_f << 8, row_offsets (n_frames + 1) the frames' rows among the call's keys, perm / run_starts what
        sort_pairs / pcc_unique_rows returned for those keys, points[f] frame f's points after the merge.  A list of
        n_frames bytes objects.  version=2 (pcc_attr_encode_frames_v2): the blobs whose coarser levels of detail are
        prefixes; `keys` the call's distinct sorted keys on the device (what octree_encode_frames took) and their
        key_shift.  n_kept (pcc_attr_encode_frames_kept): the call dropped rows; row_offsets still count every input row,
        n_kept of the sorted keys belong to kept rows.  max_error = e > 0 (pcc_attr_encode_frames_nl): the near-lossless
        kind of that version, blob version 4 (for 1) or 7 (for 2), no decoded value off by more than e.  cross
        (pcc_attr_encode_frames_cross): one cross-channel mask per frame, bit ch - 1 set where channel ch is coded
        against channel ch - 1 (include/pcc.h has the rule) -> blob versions 8, 11, 13, 14 for 1, 2, 4, 7; a frame whose
        mask is 0 gets its plain kind, and so does every frame with cross=None or all masks 0.  qstep = q > 0
        (pcc_attr_encode_frames_transform): the transform-coded kind, blob version 19, with `keys` and key_shift as
        version 2 takes them; `version` is not read, and max_error or a cross-channel mask beside it raise ValueError.
        qstep a sequence of up to 4 integers, or colour=1 beside any qstep (pcc_attr_encode_frames_transform2): blob
        version 21, one step per channel (a frame reads its first c_f; an integer serves every channel) and, with
        colour=1, the luma / chroma transform in front of the lift (include/pcc.h has the rule); the library checks both.
        scalable_to = K beside a qstep (pcc_attr_encode_frames_transform3): blob version 22, version 21 under weights a
        decoder at a cut can form, its levels of detail 0 .. K prefixes of the blob; the library checks K.
        A byte target per frame for versions 19 and 21 is a call of its own, attr_encode_frames_rate: it takes these
        arguments and writes the blob this call writes at the steps it chooses."""
        coding = AttrCoding.of(version, max_error, cross, qstep, colour, scalable_to)
        return self._attr_encode(coding, values, value_offsets, formats, row_offsets, points, perm, run_starts, n_unique, keys,
                                 key_shift, n_kept)[0]

    def attr_encode_frames_rate(self, values, value_offsets, formats, row_offsets, points, perm, run_starts, n_unique, keys,
                                key_shift, n_kept, qstep, colour, targets, scratch_limit=0, cap=None):
        """attr_encode_frames(..., qstep=, colour=) under a byte target per frame (pcc_attr_encode_frames_rate;
        include/pcc.h has the ladder and the search): blob f is the version 19 (an integer qstep without colour) or 21
        blob of the coarsened steps that the search chooses for targets[f] >= 1, qstep itself being the finest.  ->
        (blobs, rungs): rungs[f] the rung of the ladder frame f got (rate_ladder), -1 for a frame without points.  A
        frame that no rung brings under its target gets the last rung and is longer than its target.  scratch_limit
        (bytes; 0: the library's default, 1 GiB) bounds the scratch of the candidate rows; bytes and rungs do not depend
        on it.  cap: the room for the blobs (None: what attr_encode_frames takes)."""
        coding = AttrCoding.of(qstep=qstep, colour=colour, targets=targets, scratch_limit=scratch_limit)
        return self._attr_encode(coding, values, value_offsets, formats, row_offsets, points, perm, run_starts, n_unique, keys,
                                 key_shift, n_kept, cap)

    def _attr_encode(self, coding, values, value_offsets, formats, row_offsets, points, perm, run_starts, n_unique, keys, key_shift,
                     n_kept, cap=None):
        """the one binding of the eleven attribute encode entry points: the arrays of a call as attr_encode_frames takes
        them, and the AttrCoding that says which blobs to write -> (blobs, rungs), rungs None without a byte target"""
        c, nf = coding, len(formats)
        if c.cross is not None and len(c.cross) != nf:
            raise ValueError(f"{len(c.cross)} cross-channel masks for {nf} frames")
        if c.targets is not None and len(c.targets) != nf:
            raise ValueError(f"{len(c.targets)} targets for {nf} frames")
        if cap is None:
            cap = 0
            for fmt, n in zip(formats, points):
                bpv, ch = fmt & 0xFF, fmt >> 8
                cap += 96 + 2 * 80 * bpv * ch + 388 * (n // 64 + 1) + 32 * bpv * ch * n
        out = np.empty(max(int(cap), 1), dtype=np.uint8)
        offs = (C.c_int64 * (nf + 1))()
        kind = c.entry(n_kept is not None)
        versioned = kind in ("_kept", "_nl", "_cross")      # the plain family: the version behind ctx, keys for version 2 alone
        args = [self.ctx, _ptr(values), (C.c_int64 * nf)(*value_offsets), (C.c_int32 * nf)(*formats), (C.c_int64 * (nf + 1))(*row_offsets),
                (C.c_int64 * nf)(*points), nf, _ptr(perm), _ptr(run_starts), n_unique]
        if versioned:
            args.insert(1, c.version)
        if kind == "_v2":
            args += [_ptr(keys), int(key_shift)]
        elif kind:
            args += [-1 if n_kept is None else int(n_kept), None if versioned and c.version == 1 else _ptr(keys), int(key_shift)]
        four = None if c.steps is None else (C.c_int32 * 4)(*c.four(c.steps))
        args += {"": (), "_v2": (), "_kept": (), "_nl": (c.max_error,),
                 "_nbr": (None if c.cross is None or not any(c.cross) else (C.c_int32 * nf)(*c.cross),),
                 "_nbr_nl": (c.max_error, None if c.cross is None or not any(c.cross) else (C.c_int32 * nf)(*c.cross)),
                 "_cross": (c.max_error, None if c.cross is None else (C.c_int32 * nf)(*c.cross)),
                 "_transform": (c.steps and c.steps[0],), "_transform2": (four, c.colour), "_transform3": (four, c.colour, c.scalable_to),
                 "_rate": (four, int(c.per_channel), c.colour, None if c.targets is None else (C.c_int64 * nf)(*c.targets),
                           c.scratch_limit)}[kind]
        rungs = (C.c_int32 * nf)() if kind == "_rate" else None
        name = "pcc_attr_encode_frames" + kind
        check(getattr(self.lib, name)(*args, _np_ptr(out), int(cap), offs, *(() if rungs is None else (rungs,))), name)
        return [out[offs[f]:offs[f + 1]].tobytes() for f in range(nf)], None if rungs is None else list(rungs)

    @staticmethod
    def attr_rate_ladder(qstep, bpv, channels):
        """the ladder of steps that a byte target walks from the base steps `qstep` (an integer, or one step per channel)
        for values of bpv bytes and `channels` channels (pcc_attr_rate_ladder, host only): a list of J tuples"""
        out = (C.c_int32 * 256)()
        J = C.c_int32(0)
        check(_abi.lib().pcc_attr_rate_ladder((C.c_int32 * 4)(*AttrCoding.four(qstep)), int(channels), int(bpv), out, C.byref(J)), "pcc_attr_rate_ladder")
        return [tuple(out[4 * j + ch] for ch in range(int(channels))) for j in range(J.value)]

    @staticmethod
    def attr_lod_info(blob, lod):
        """(bytes, values) of level of detail `lod` (0 .. 15) of a version-2 attribute blob, or of one of version 7, 11, 14
        or 22 (22: up to its scalable_to) (pcc_attr_lod_info, host only): the shortest prefix that decodes at that level,
        and the rows it gives.  `blob` may itself be a prefix
        that reaches the last needed chunk's length table."""
        buf = np.frombuffer(blob, dtype=np.uint8)
        nbytes, values = C.c_int64(0), C.c_int64(0)
        check(_abi.lib().pcc_attr_lod_info(_np_ptr(buf) if buf.shape[0] else None, buf.shape[0], int(lod),
                                           C.byref(nbytes), C.byref(values)), "pcc_attr_lod_info")
        return nbytes.value, values.value

    @staticmethod
    def attr_info(blob):
        """what the head of an attribute blob of any kind says (pcc_attr_info, host only): a dict of version (1, 2, 4,
        7, their cross-channel forms 8, 11, 13, 14, or the transform-coded 19), bpv, channels, points, max_error (0:
        lossless, and version 19), scalable, lod (the sender's); for the cross-channel kinds also cross_channel, the tuple
        of channels coded against the channel before them (pcc_attr_cross_mask); for version 19 also qstep
        (pcc_attr_qstep; 0 in a blob without points); for version 21 qstep, a tuple of one step per channel, and colour,
        "ycocg" or None (pcc_attr_transform_info; zeros and None in a blob without points); for version 22 those two and
        scalable_to, its deepest level-of-detail prefix (pcc_attr_scalable_to; 0 in a blob without points); for versions
        25, 26, 28 and 31 also predictor, the string "neighbours" (pcc_attr_info's version byte; 28 and 31 with their
        max_error >= 1)"""
        buf = np.frombuffer(blob, dtype=np.uint8)
        v = [C.c_int32(0) for _ in range(6)]
        n = C.c_int64(0)
        check(_abi.lib().pcc_attr_info(_np_ptr(buf) if buf.shape[0] else None, buf.shape[0], C.byref(v[0]), C.byref(v[1]),
                                       C.byref(v[2]), C.byref(n), C.byref(v[3]), C.byref(v[4]), C.byref(v[5])), "pcc_attr_info")
        info = {"version": v[0].value, "bpv": v[1].value, "channels": v[2].value, "points": n.value,
                "max_error": v[3].value, "scalable": bool(v[4].value), "lod": v[5].value}
        if info["version"] in ATTR_CROSS_KINDS:
            m = C.c_int32(0)
            check(_abi.lib().pcc_attr_cross_mask(_np_ptr(buf), buf.shape[0], C.byref(m)), "pcc_attr_cross_mask")
            info["cross_channel"] = tuple(ch for ch in range(1, 4) if m.value >> (ch - 1) & 1)
        if info["version"] in ATTR_NEIGHBOUR_KINDS:
            info["predictor"] = "neighbours"
        if info["version"] == ATTR_TRANSFORM_KIND:
            q = C.c_int32(0)
            check(_abi.lib().pcc_attr_qstep(_np_ptr(buf), buf.shape[0], C.byref(q)), "pcc_attr_qstep")
            info["qstep"] = q.value
        if info["version"] in (ATTR_COLOUR_KIND, ATTR_SCALABLE_TRANSFORM_KIND):
            col, steps = C.c_int32(0), (C.c_int32 * 4)()
            check(_abi.lib().pcc_attr_transform_info(_np_ptr(buf), buf.shape[0], C.byref(col), steps), "pcc_attr_transform_info")
            info["qstep"] = tuple(int(q) for q in steps[:info["channels"]])
            info["colour"] = "ycocg" if col.value else None
        if info["version"] == ATTR_SCALABLE_TRANSFORM_KIND:
            k = C.c_int32(0)
            check(_abi.lib().pcc_attr_scalable_to(_np_ptr(buf), buf.shape[0], C.byref(k)), "pcc_attr_scalable_to")
            info["scalable_to"] = k.value
        return info

    def attr_decode_frames(self, blobs, points=None, device=False, lod=None, cells=None):
        """attribute blobs -> one [n_f, c_f] array per blob in its dtype (uint8 / uint16), row i belonging to decoded
        point i (pcc_attr_decode_frames: versions 1, 4, 8 and 13, one version per call): numpy arrays, or views of one device
        tensor (device=True).  points[f]
        (optional): frame f's geometry point count, checked against the blob before anything is launched.
        lod = k (0 .. 15) with cells (pcc_attr_decode_frames_lod): blobs of version 2, or of 7, 11, 14, 25, 26, 28 or 31, or prefixes of them (attr_lod_info)
        -> row j the value of the j-th cell of the frame's geometry at that lod; lod = 0 with cells also reads whole
        blobs of version 19 or of version 21, whose transform needs the frame's keys (a call of them at lod > 0: PccError), and lod = 0 .. K reads blobs of version 22 or their prefixes (K: every blob's scalable_to); `cells` the device tensors
        octree_decode_frames(..., device=True, lod=k) returned for the same frames (views of one tensor)."""
        nb = len(blobs)
        if nb == 0:
            return []
        bufs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
        ptrs = (C.c_void_p * nb)(*[b.ctypes.data if b.shape[0] else None for b in bufs])
        lens = (C.c_int64 * nb)(*[b.shape[0] for b in bufs])
        offs = (C.c_int64 * (nb + 1))()
        fmt = (C.c_int32 * nb)()
        if lod is None:
            name = "pcc_attr_decode_frames"
            pts = (C.c_int64 * nb)(*points) if points is not None else None
            call = lambda *a: self.lib.pcc_attr_decode_frames(self.ctx, ptrs, lens, nb, pts, *a, offs, fmt)
            rows = [struct.unpack_from("<I", b, 4)[0] if len(b) >= 8 else 0 for b in blobs]
        else:
            name = "pcc_attr_decode_frames_lod"
            if cells is None or len(cells) != nb:
                raise ValueError("attr_decode_frames at a lod needs the decoded cells of every frame")
            rows = [int(c.shape[0]) for c in cells]
            base = None
            cell_offs = [0]
            for c in cells:      # the frames' cells must lie behind one another, as octree_decode_frames leaves them
                if c.shape[0]:
                    if not (c.is_cuda and c.dtype == torch.int32 and c.is_contiguous()):
                        raise ValueError("the cells must be contiguous int32 device tensors")
                    if base is None:
                        base = c.data_ptr() - 12 * cell_offs[-1]
                    if c.data_ptr() != base + 12 * cell_offs[-1]:
                        raise ValueError("the cells of the frames must be consecutive views of one device tensor")
                cell_offs.append(cell_offs[-1] + int(c.shape[0]))
            coffs = (C.c_int64 * (nb + 1))(*cell_offs)
            call = lambda *a: self.lib.pcc_attr_decode_frames_lod(self.ctx, ptrs, lens, nb, int(lod), C.c_void_p(base), coffs,
                                                                  *a, offs, fmt)
        out = self._sized_output(call, name, offs, lambda total: (max(total, 16),), torch.uint8, device)
        res = []
        for f in range(nb):
            bpv, c = fmt[f] & 0xFF, fmt[f] >> 8
            n = rows[f]
            seg = out[offs[f]:offs[f] + n * c * bpv]
            if device:
                res.append(seg.view(torch.uint8 if bpv == 1 else torch.uint16).reshape(n, c))
            else:
                res.append(seg.view(np.uint8 if bpv == 1 else np.uint16).reshape(n, c))
        return res


# the kinds of attribute blob by version byte (csrc/attr_blob.h): those one lane run predicts through, which decode at
# lod 0 only (pcc_attr_decode_frames), and the cross-channel forms 8, 11, 13, 14 of 1, 2, 4, 7
ATTR_RUN_KINDS = (1, 4, 8, 13)
ATTR_CROSS_KINDS = (8, 11, 13, 14, 26, 31)
# scalable under the predictor from 3-D neighbours: lossless and its cross-channel form, bounded-error (a closed loop
# over decoded values) and its cross-channel form; decoded as version 2's family is
ATTR_NEIGHBOUR_KINDS = (25, 26, 28, 31)
# the transform-coded kind: it decodes against the cells as version 2's family does, but at lod 0 only
ATTR_TRANSFORM_KIND = 19
# version 19 with a colour transform and one step per channel: decoded as version 19 is
ATTR_COLOUR_KIND = 21
ATTR_TRANSFORM_KINDS = (ATTR_TRANSFORM_KIND, ATTR_COLOUR_KIND)
# version 21 under weights a decoder at a cut can form: decodes at lod 0 .. its scalable_to, from prefixes
ATTR_SCALABLE_TRANSFORM_KIND = 22
# what a value of an attribute source is (PCC_ATTR_SRC_* of include/pcc.h), by the name of its dtype
ATTR_SRC_KINDS = {"uint8": 0, "uint16": 1, "float32": 2, "float64": 3}

class AttrCoding(NamedTuple):
    """What kind of attribute blob an encode call writes, resolved and normalised once: what travels from
    GeometryCodec.compress to the one binding of the encode entry points, Runtime._attr_encode."""
    version: int = 1               # 1 or 2: the plain family (2: coarser levels of detail are prefixes)
    max_error: int = 0             # e > 0: the near-lossless kind of that version
    cross: tuple = None            # one cross-channel mask per frame, or None
    steps: tuple = None            # transform-coded: 1 to 4 quantiser steps, an integer step four times; None: not
    per_channel: bool = False      # False: the one integer step of version 19; True: versions 21 / 22, a step per channel
    colour: int = 0                # 1: the luma / chroma transform in front of the lift
    scalable_to: int = None        # K: version 22, levels of detail 0 .. K are prefixes
    targets: tuple = None          # a byte target per frame: the steps are the finest the search may choose
    scratch_limit: int = 0         # bytes of scratch for the candidates of a byte target; 0: the library's default
    neighbours: bool = False       # versions 25 / 26: version 2's family under the predictor from 3-D neighbours
    neighbours_nl: bool = False    # versions 28 / 31: that predictor in a closed loop, every error within max_error >= 1

    @staticmethod
    def four(qstep, what=""):
        """the four steps the library takes: an integer serves all four channels, a sequence is padded with zeros to 4"""
        steps = [int(qstep)] * 4 if isinstance(qstep, (int, np.integer)) else [int(q) for q in qstep]
        if not 1 <= len(steps) <= 4:
            raise ValueError(f"{what}{len(steps)} steps, at most 4")
        return steps + [0] * (4 - len(steps))

    @classmethod
    def of(cls, version=1, max_error=0, cross=None, qstep=0, colour=None, scalable_to=None, targets=None, scratch_limit=0,
           neighbours=False, neighbours_nl=False):
        """the record of the loose keywords of Runtime.attr_encode_frames and attr_encode_frames_rate; what contradicts
        itself raises ValueError here, what needs the number of frames in Runtime._attr_encode"""
        if version not in (1, 2):
            raise ValueError(f"attribute blob version {version!r}: 1 or 2")
        one = isinstance(qstep, (int, np.integer))      # one integer step
        if scalable_to is not None and one and int(qstep) == 0:
            raise ValueError("scalable_to (attribute blob version 22) needs qstep")
        per_channel = bool(colour) or scalable_to is not None or not one
        steps = None
        if per_channel or int(qstep) or targets is not None:
            steps = tuple(cls.four(qstep, "attribute blob version 21: ")[:4 if one else len(qstep)])
        if steps is not None and (int(max_error) or (cross is not None and any(cross))):
            raise ValueError("qstep (attribute blob versions 19 and 21) has no near-lossless and no cross-channel form")
        if neighbours and (steps is not None or int(max_error) or scalable_to is not None):
            raise ValueError("the predictor from 3-D neighbours (attribute blob versions 25 and 26) is lossless: it has no "
                             "transform-coded form, and its near-lossless form is neighbours_nl (versions 28 and 31)")
        if neighbours_nl and (neighbours or steps is not None or int(max_error) < 1 or scalable_to is not None or targets is not None):
            raise ValueError("the bounded-error predictor from 3-D neighbours (attribute blob versions 28 and 31) needs max_error "
                             ">= 1 and has no lossless record (that is neighbours), no transform-coded form and no byte target")
        return cls(version, int(max_error), None if cross is None else tuple(int(m) for m in cross), steps, per_channel,
                   int(colour or 0), None if scalable_to is None else int(scalable_to),
                   None if targets is None else tuple(int(t) for t in targets), int(scratch_limit), bool(neighbours),
                   bool(neighbours_nl))

    @property
    def qstep(self):
        """the qstep keyword that gives these steps"""
        return 0 if self.steps is None else self.steps if self.per_channel else self.steps[0]

    def entry(self, dropped):
        """which of the eleven entry points codes this record, as the suffix of pcc_attr_encode_frames; `dropped`: the call
        left rows out (n_kept).  The first match wins."""
        for hit, kind in ((self.neighbours_nl, "_nbr_nl"),
                          (self.neighbours, "_nbr"),
                          (self.targets is not None, "_rate"),
                          (self.scalable_to is not None, "_transform3"),
                          (self.steps is not None and self.per_channel, "_transform2"),
                          (self.steps is not None, "_transform"),
                          (self.cross is not None and any(self.cross), "_cross"),      # all masks 0: the plain kinds below
                          (self.max_error, "_nl"),
                          (dropped, "_kept"),
                          (self.version == 1, "")):
            if hit:
                return kind
        return "_v2"


OCTREE_V2_MIN_LEAVES = 65536     # include/pcc.h PCC_OCTREE_V2_MIN_LEAVES
OCTREE_V3_MIN_LEAVES = 8192      # include/pcc.h PCC_OCTREE_V3_MIN_LEAVES


# ---------------------------------------------------------------- GPU coder (container version 1)
class RansDev:
    """a CDF set in HBM for the interleaved rANS coder on the GPU (pcc_rans_dev_*, csrc/rans_gpu.hip)"""

    def __init__(self, cdfs, sizes, offsets):
        self.lib = _abi.lib()
        cdfs = np.ascontiguousarray(cdfs, dtype=np.int32)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.handle = self.lib.pcc_rans_dev_create(_np_ptr(cdfs), cdfs.shape[1], _np_ptr(sizes), _np_ptr(offsets),
                                                   cdfs.shape[0])
        if not self.handle:
            raise PccError(-1, "pcc_rans_dev_create", self.lib.pcc_last_error().decode(errors="replace"))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pcc_rans_dev_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, rt, sym, idx=None, idx_run=1):
        """sym: int32 device tensor [S, n]; idx: uint8 device tensor [S, n] or None (table = position // idx_run).
        Returns the S streams as bytes."""
        assert sym.is_cuda and sym.dtype == torch.int32 and sym.dim() == 2 and sym.is_contiguous()
        s, n = sym.shape
        if idx is not None:
            assert idx.is_cuda and idx.dtype == torch.uint8 and idx.shape == sym.shape and idx.is_contiguous()
        cap = (int(self.lib.pcc_rans_dev_bound(n)) + 3) // 4 * 4
        cap = min(cap, 4 * (4 + n + 4096 + 130 * (n // 32768 + 1)) * 3)     # generous; the call reports if it is not
        out = rt.empty((s, cap), torch.uint8)
        lens = (C.c_int64 * s)()
        check(self.lib.pcc_rans_encode_dev(rt.ctx, self.handle, _ptr(sym), _ptr(idx) if idx is not None else None,
                                           idx_run, n, s, _ptr(out), cap, lens), "pcc_rans_encode_dev")
        host = out.cpu().numpy()
        return [host[i, :lens[i]].tobytes() for i in range(s)]

    def decode(self, rt, data, n, idx=None, idx_run=1):
        """data: bytes of one stream; returns the int32 device tensor [n] (raises on a malformed stream)"""
        buf = np.frombuffer(data, dtype=np.uint8)
        hn, ht, hc = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.pcc_rans_stream_info(_np_ptr(buf), buf.shape[0], C.byref(hn), C.byref(ht), C.byref(hc)),
              "pcc_rans_stream_info")
        if hn.value != n:
            raise PccError(-5, "RansDev.decode", f"stream holds {hn.value} symbols, {n} expected")
        d_in = rt.to_device(buf.copy())
        sym = rt.empty((n,), torch.int32)
        status = torch.zeros(1, dtype=torch.int32, device=sym.device)
        check(self.lib.pcc_rans_decode_dev(rt.ctx, self.handle, _ptr(d_in), buf.shape[0], n, ht.value, hc.value,
                                           _ptr(idx) if idx is not None else None, idx_run, _ptr(sym), _ptr(status)),
              "pcc_rans_decode_dev")
        rt.sync()
        st = int(status.item())
        if st:
            raise PccError(-5, "pcc_rans_decode_dev", f"malformed interleaved rANS stream (status {st})")
        return sym


# ---------------------------------------------------------------- host coders (no ctx)
def rans_encode_multi(sym, idx, cdfs, sizes, offsets):
    """sym/idx: numpy [S, n], either (int32, int32) or the compact (int16, uint8);
    returns list of S byte strings"""
    lib = _abi.lib()
    s, n = sym.shape
    if sym.dtype == np.int16 and idx.dtype == np.uint8:
        fn, name = lib.pcc_rans_encode_multi16, "pcc_rans_encode_multi16"
    elif sym.dtype == np.int32 and idx.dtype == np.int32:
        fn, name = lib.pcc_rans_encode_multi, "pcc_rans_encode_multi"
    else:
        raise TypeError(f"rans_encode_multi: unsupported dtypes {sym.dtype}/{idx.dtype}")
    lens = (C.c_int64 * s)()
    cap = 2 * n + 4096                      # in-range symbols cost <= 16 bits each
    for _ in range(2):
        out = np.empty((s, cap), dtype=np.uint8)
        rc = fn(_np_ptr(sym), _np_ptr(idx), n, s, _np_ptr(cdfs), cdfs.shape[1], _np_ptr(sizes), _np_ptr(offsets),
                cdfs.shape[0], _np_ptr(out), cap, lens)
        if rc != _abi.PCC_E_NOMEM:
            break
        cap = 48 * n + 4096                 # escape-heavy input: absolute worst case
    check(rc, name)
    return [out[i, :lens[i]].tobytes() for i in range(s)]


def rans_encode(sym, idx, cdfs, sizes, offsets):
    return rans_encode_multi(sym.reshape(1, -1), idx.reshape(1, -1), cdfs, sizes, offsets)[0]


def rans_decode(data, idx, cdfs, sizes, offsets, out=None):
    """idx: int32 or uint8 numpy [n]; returns int32 symbols (written into `out` if given)"""
    lib = _abi.lib()
    n = idx.shape[0]
    buf = np.frombuffer(data, dtype=np.uint8)
    sym = out if out is not None else np.empty(n, dtype=np.int32)
    assert sym.dtype == np.int32 and sym.shape[0] == n
    if idx.dtype == np.uint8:
        fn, name = lib.pcc_rans_decode8, "pcc_rans_decode8"
    else:
        fn, name = lib.pcc_rans_decode, "pcc_rans_decode"
        assert idx.dtype == np.int32
    check(fn(_np_ptr(buf), buf.shape[0], _np_ptr(idx), n, _np_ptr(cdfs), cdfs.shape[1], _np_ptr(sizes),
             _np_ptr(offsets), cdfs.shape[0], _np_ptr(sym)), name)
    return sym


def octree_pack(occ, level_n, n_points, origin):
    lib = _abi.lib()
    depth = len(level_n)
    cap = 64 + 2 * len(occ) + 16
    out = np.empty(cap, dtype=np.uint8)
    ln = (C.c_int64 * max(depth, 1))(*level_n)
    org = (C.c_int * 3)(*[int(v) for v in origin])
    length = C.c_int64(0)
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    check(lib.pcc_octree_pack(_np_ptr(occ) if len(occ) else C.c_void_p(0), ln, depth, n_points, org,
                              _np_ptr(out), cap, C.byref(length)), "pcc_octree_pack")
    return out[:length.value].tobytes()


def octree_unpack(blob):
    lib = _abi.lib()
    buf = np.frombuffer(blob, dtype=np.uint8)
    n = C.c_int64(0)
    depth = C.c_int(0)
    org = (C.c_int * 3)()
    check(lib.pcc_octree_peek(_np_ptr(buf), buf.shape[0], C.byref(n), C.byref(depth), org), "pcc_octree_peek")
    pts = np.empty((n.value, 3), dtype=np.int32)
    if n.value:
        check(lib.pcc_octree_unpack(_np_ptr(buf), buf.shape[0], _np_ptr(pts), n.value), "pcc_octree_unpack")
    return pts
