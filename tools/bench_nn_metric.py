#!/usr/bin/env python3
"""GeometryCodec.distortion (exact nearest neighbours on the device, csrc/nn.hip) against the host path it replaces,
metrics.d1_psnr (scipy's k-d tree in float64 on the box's CPU share), in ms per call, both directions of the metric.

Cases (seeded), the paths alternating in one process, the order reversed every round, median of REPS:
  room     the 1M-point room (workloads.room) against the centres of its lod = 1 and lod = 2 cells: "host" (k-d tree),
           "device_from_host" (distortion of numpy frames), "device_from_device" (distortion of device tensors)
  sweeps   32 LiDAR sweeps (workloads.lidar_sweep(seed=s)) against their lod = 2 centres: "host_loop" (32 k-d tree
           calls), "device_loop" (32 one-frame distortion calls), "device_one_call" (one call of 32 frames)
Every timed case is checked first: the two paths agree in both mse to relative 1e-12.

Also, per case, the nodes a query tries (mean, max; cells tested and points measured) from the traversal replayed on
the host (pcc_nn_replay_host, the kernel's search function compiled for the host), both directions.

--calls N --case room|sweeps: only N device calls of that case (from device tensors; one call of 32 for the sweeps),
for a rocprofv3 --kernel-trace --stats run of its own; --kernel-stats room=<csv>,sweeps=<csv> copies the k_nn_frames
rows of such runs' kernel_stats files into the result.  Writes one JSON object (stdout, --out)."""
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


def centres(codec, frames, k):
    cells = codec.decompress(codec.compress(frames), lod=k)
    return [((c << k) + ((1 << k) >> 1)).astype(np.int32) for c in cells]


def agree(rep, host):
    for r, (_, e_ab, e_ba) in zip(rep, host):
        assert abs(r["mse_ab"] - e_ab) <= 1e-12 * e_ab and abs(r["mse_ba"] - e_ba) <= 1e-12 * e_ba, (r, e_ab, e_ba)


def timed(variants, reps):
    names = list(variants)
    t = {k: [] for k in names}
    for it in range(reps + 1):      # round 0 warms up
        for k in (names if it % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            variants[k]()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if it:
                t[k].append(t1 - t0)
    return {k: round(1e3 * float(np.median(v)), 3) for k, v in t.items()}


def morton_keys(points, frame=0):
    def spread(v):
        x = v.astype(np.uint64) & np.uint64(0xFFFF)
        for s, m in ((16, 0x0000FF0000FF), (8, 0x00F00F00F00F), (4, 0x0C30C30C30C3), (2, 0x249249249249)):
            x = (x | (x << np.uint64(s))) & np.uint64(m)
        return x
    p = np.asarray(points, dtype=np.int64) + 32768
    return (np.uint64(frame) << np.uint64(48)) | (spread(p[:, 0]) << np.uint64(2)) | (spread(p[:, 1]) << np.uint64(1)) | spread(p[:, 2])


def nodes_tried(lib, a, b):
    """{"a_to_b", "b_to_a"}: (mean, max) nodes per query of the traversal, replayed on the host"""
    out = {}
    for name, q, r in (("a_to_b", a, b), ("b_to_a", b, a)):
        qk = np.sort(morton_keys(q))
        rk = np.unique(morton_keys(r))
        nodes = np.zeros(qk.shape[0], np.uint32)
        rc = lib.pcc_nn_replay_host(qk.ctypes.data, qk.shape[0], rk.ctypes.data, rk.shape[0], None, None, nodes.ctypes.data)
        assert rc == 0
        out[name] = {"mean": round(float(nodes.mean()), 2), "max": int(nodes.max())}
    return out


def kernel_rows(path):
    with open(path, newline="") as f:
        return [{"kernel": "k_nn_frames", "calls": int(r["Calls"]), "total_ms": round(int(r["TotalDurationNs"]) / 1e6, 3),
                 "avg_ms": round(float(r["AverageNs"]) / 1e6, 4), "min_ms": round(int(r["MinNs"]) / 1e6, 4),
                 "max_ms": round(int(r["MaxNs"]) / 1e6, 4)} for r in csv.DictReader(f) if "k_nn_frames" in r["Name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "9")))
    ap.add_argument("--sweeps", type=int, default=32)
    ap.add_argument("--case", default="all", choices=["all", "room", "sweeps"])
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    metrics = importlib.import_module(PKG + ".metrics")
    lib = importlib.import_module(PKG + "._abi").lib()
    codec = pkg.GeometryCodec()
    dev = codec.rt.device
    to_dev = lambda frames: [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "host_threads": importlib.import_module(PKG + "._abi").host_cpu_budget()}

    if args.case in ("all", "room"):
        pts = wl.room()["points"].astype(np.int32)
        peak = metrics.peak_of(pts)
        res["room"] = {"points": int(pts.shape[0]), "peak": int(peak)}
        for k in (1, 2):
            ctr = centres(codec, [pts], k)[0]
            d_pts, d_ctr = to_dev([pts]), to_dev([ctr])
            torch.cuda.synchronize()
            if args.calls:
                if k == 2:
                    for _ in range(args.calls):
                        codec.distortion(d_pts, d_ctr, peak=peak)
                continue
            host = metrics.d1_psnr(pts, ctr, peak)
            rep = codec.distortion([pts], [ctr], peak=peak)
            agree(rep, [host])
            agree(codec.distortion(d_pts, d_ctr, peak=peak), [host])
            row = timed({"host": lambda: metrics.d1_psnr(pts, ctr, peak),
                         "device_from_host": lambda: codec.distortion([pts], [ctr], peak=peak),
                         "device_from_device": lambda: codec.distortion(d_pts, d_ctr, peak=peak)}, args.reps)
            row.update({"cells": int(ctr.shape[0]), "mse_ab": rep[0]["mse_ab"], "mse_ba": rep[0]["mse_ba"],
                        "d1_psnr": round(rep[0]["d1_psnr"], 4), "nodes_per_query": nodes_tried(lib, pts, ctr)})
            res["room"][f"lod{k}"] = row
            print(f"room lod{k}", json.dumps(row), flush=True)

    if args.case in ("all", "sweeps"):
        frames = [wl.lidar_sweep(seed=s)["points"].astype(np.int32) for s in range(args.sweeps)]
        ctr = centres(codec, frames, 2)
        peak = 65535
        d_frames, d_ctr = to_dev(frames), to_dev(ctr)
        torch.cuda.synchronize()
        if args.calls:
            for _ in range(args.calls):
                codec.distortion(d_frames, d_ctr, peak=peak)
        else:
            host = [metrics.d1_psnr(a, b, peak) for a, b in zip(frames, ctr)]
            rep = codec.distortion(frames, ctr, peak=peak)
            agree(rep, host)
            agree([codec.distortion([a], [b], peak=peak)[0] for a, b in zip(frames, ctr)], host)
            row = timed({"host_loop": lambda: [metrics.d1_psnr(a, b, peak) for a, b in zip(frames, ctr)],
                         "device_loop": lambda: [codec.distortion([a], [b], peak=peak) for a, b in zip(frames, ctr)],
                         "device_one_call": lambda: codec.distortion(frames, ctr, peak=peak),
                         "device_one_call_from_device": lambda: codec.distortion(d_frames, d_ctr, peak=peak)}, args.reps)
            row.update({"sweeps": len(frames), "points": int(sum(f.shape[0] for f in frames)),
                        "cells": int(sum(c.shape[0] for c in ctr)), "mse_ab_sweep0": rep[0]["mse_ab"],
                        "mse_ba_sweep0": rep[0]["mse_ba"], "nodes_per_query_sweep0": nodes_tried(lib, frames[0], ctr[0])})
            res["sweeps"] = row
            print("sweeps", json.dumps(row), flush=True)
    codec.close()
    if args.calls:
        return
    if args.kernel_stats:
        res["kernel"] = {name: kernel_rows(path) for name, path in (item.split("=", 1) for item in args.kernel_stats.split(","))}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
