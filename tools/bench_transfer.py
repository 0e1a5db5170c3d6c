#!/usr/bin/env python3
"""GeometryCodec.transfer (attribute transfer onto another geometry, csrc/transfer.hip), ms per call.

Cases (seeded):
  room     workloads.room(1_000_000) with its RGB onto the centres of its lod-2 cells
  zed      the first recorded camera frame of tests/golden/zed_seq25.npz with its RGB onto its lod-1 centres
  sweeps   eight LiDAR sweeps (workloads.lidar_sweep(seed=s)) with workloads.lidar_intensity onto their lod-1 centres,
           one call of eight frames
  paths    "from_host" (numpy frames -> numpy), "from_device" (device tensors -> device tensors)
Median of 10 calls behind 2 warm-ups.  Beside each case: the bytes the accumulate kernel moves (per source row its
key, its target row and its values; per target the channels + 1 uint64 accumulator words once) and what a plain device
copy of that many bytes takes (tools/hbm_copy.py's method: half read, half written, events around 20 copies).

--calls N: only N device calls per case, in the order of --case, for a rocprofv3 --kernel-trace --stats run of its own;
--kernel-trace <csv> reads that run's kernel trace back: every call dispatches k_nn_frames twice (the backward search,
then the forward one), k_transfer_accumulate and k_transfer_finish once, so dispatch i of a kernel belongs to case
i // N.  Writes one JSON object (stdout, --out)."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "demo-learned-point-cloud-compression_amd"
CASES = ("room", "zed", "sweeps")


def centres(codec, frames, k):
    cells = codec.decompress(codec.compress(frames), lod=k)
    return [((c << k) + ((1 << k) >> 1)).astype(np.int32) for c in cells]


def inputs(codec, wl, case):
    """(source frames int32, attributes, target frames int32)"""
    if case == "room":
        fr = wl.room(1_000_000)
        frames, attrs, k = [fr["points"].astype(np.int32)], [np.rint(fr["colors"] * 255.0).astype(np.uint8)], 2
    elif case == "zed":
        with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
            frames, attrs, k = [f["points_0"].astype(np.int32)], [np.ascontiguousarray(f["colors_u8_0"])], 1
    else:
        frames = [wl.lidar_sweep(seed=s)["points"].astype(np.int32) for s in range(8)]
        attrs, k = [wl.lidar_intensity(p, seed=s) for s, p in enumerate(frames)], 1
    return frames, attrs, centres(codec, frames, k)


def median_ms(call, reps=10, warmups=2):
    t = []
    for it in range(warmups + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if it >= warmups:
            t.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(t)), 3)


def plain_copy_ms(nbytes):
    n = max(nbytes // 8, 1)      # n float32 read, n written
    x = torch.empty(n, dtype=torch.float32, device="cuda").normal_()
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        y.copy_(x)
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / 20, 5)


def accumulate_bytes(attrs, n_s, n_t):
    bpv = max(a.dtype.itemsize for a in attrs)
    channels = max(1 if a.ndim == 1 else a.shape[1] for a in attrs)
    channels = 4 if bpv == 1 or channels > 2 else 2      # the call's common row (GeometryCodec.transfer)
    return n_s * (8 + 4 + channels * bpv) + n_t * (channels + 1) * 8, channels, bpv


def trace_rows(path, cases, calls):
    """per case the median device time in ms of the two searches, of accumulate and of finish"""
    per = {"k_nn_frames": [], "k_transfer_accumulate": [], "k_transfer_finish": []}
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for name in per:
            if name in r["Kernel_Name"]:
                per[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    assert len(per["k_transfer_accumulate"]) == len(per["k_transfer_finish"]) == len(cases) * calls, {k: len(v) for k, v in per.items()}
    assert len(per["k_nn_frames"]) == 2 * len(cases) * calls
    med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
    out = {}
    for i, case in enumerate(cases):
        nn = per["k_nn_frames"][2 * i * calls:2 * (i + 1) * calls]
        out[case] = {"search_backward_ms": med(nn[0::2]), "search_forward_ms": med(nn[1::2]),
                     "accumulate_ms": med(per["k_transfer_accumulate"][i * calls:(i + 1) * calls]),
                     "finish_ms": med(per["k_transfer_finish"][i * calls:(i + 1) * calls])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all"] + list(CASES))
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-calls", type=int, default=5, help="the --calls of the run that wrote --kernel-trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    codec = pkg.GeometryCodec()
    dev = codec.rt.device
    cases = CASES if args.case == "all" else (args.case,)
    res = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmups": 2}
    for case in cases:
        frames, attrs, targets = inputs(codec, wl, case)
        d_frames = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in frames]
        d_targets = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in targets]
        torch.cuda.synchronize()
        if args.calls:
            for _ in range(args.calls):
                codec.transfer(d_frames, attrs, d_targets, output="device")
            continue
        n_s, n_t = int(sum(p.shape[0] for p in frames)), int(sum(p.shape[0] for p in targets))
        got, cnt = codec.transfer(frames, attrs, targets, return_counts=True)
        nbytes, channels, bpv = accumulate_bytes(attrs, n_s, n_t)
        row = {"frames": len(frames), "source_rows": n_s, "targets": n_t, "channels_in_call": channels, "bytes_per_value": bpv,
               "fallbacks": int(sum(int((c == 0).sum()) for c in cnt)), "shared_targets": int(sum(int((c > 1).sum()) for c in cnt)),
               "from_host_ms": median_ms(lambda: codec.transfer(frames, attrs, targets)),
               "from_device_ms": median_ms(lambda: codec.transfer(d_frames, attrs, d_targets, output="device")),
               "accumulate_bytes": nbytes, "plain_copy_same_bytes_ms": plain_copy_ms(nbytes)}
        res[case] = row
        print(case, json.dumps(row), flush=True)
    codec.close()
    if args.calls:
        return
    if args.kernel_trace:
        for case, k in trace_rows(args.kernel_trace, cases, args.trace_calls).items():
            res[case]["kernels"] = k
            res[case]["accumulate_gb_per_s"] = round(res[case]["accumulate_bytes"] / k["accumulate_ms"] / 1e6, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
