#!/usr/bin/env python3
"""Levels of detail of stored geometry blobs: what a coarser level costs in bytes and in decode time.

Workloads (seeded): one KITTI-like sweep (workloads.lidar_sweep(seed=1)), 32 sweeps (seeds 0 .. 31) in one call, one
1M-point room (workloads.room(seed=0)).  Per workload and k = 0 .. 4: the bytes of the shortest decodable prefixes
(GeometryCodec.lod_info) and their share of the blobs, the cells, and ms per frame of decompress(prefixes, lod=k) to
host arrays — every k alternating with k = 0 in one process (median of REPS; "ms_k0_beside" is k = 0 measured in the
same rounds).  Every level's result is checked against the full decode >> k.  Writes one JSON object (stdout, --out).

--only-lod K: nothing but REPS decode calls at lod K per workload (for a kernel trace of its own)."""
import argparse
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


def med_ms(v):
    return 1e3 * float(np.median(v))


def coarse(points, k):
    c = points >> k
    keep = np.ones(c.shape[0], bool)
    keep[1:] = np.any(c[1:] != c[:-1], axis=1)
    return c[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lods", default="0,1,2,3,4")
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "9")))
    ap.add_argument("--workloads", default="sweep,sweep32,room")
    ap.add_argument("--only-lod", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    lods = [int(k) for k in args.lods.split(",")]
    make = {"sweep": lambda: [wl.lidar_sweep(seed=1)["points"]],
            "sweep32": lambda: [wl.lidar_sweep(seed=s)["points"] for s in range(32)],
            "room": lambda: [wl.room(1_000_000, seed=0)["points"]]}
    codec = pkg.GeometryCodec()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "workloads": {}}
    for name in args.workloads.split(","):
        frames = make[name]()
        B = len(frames)
        blobs = codec.compress(frames)
        total = sum(len(b) for b in blobs)
        if args.only_lod is not None:
            k = args.only_lod
            pre = [b[:codec.lod_info(b, k)[0]] for b in blobs]
            for _ in range(args.reps):
                codec.decompress(pre, lod=k)
            print(f"{name}: {args.reps} decode calls at lod {k}", flush=True)
            continue
        full = codec.decompress(blobs)
        rows = {}
        for k in lods:
            info = [codec.lod_info(b, k) for b in blobs]
            pre = [b[:nb] for b, (nb, _) in zip(blobs, info)]
            got = codec.decompress(pre, lod=k)
            assert all(np.array_equal(g, coarse(p, k)) and g.shape[0] == m for g, p, (_, m) in zip(got, full, info)), (name, k)
            t = {0: [], k: []}
            for it in range(args.reps + 1):
                for kk in ((0, k) if it % 2 == 0 else (k, 0)):
                    src = blobs if kk == 0 else pre
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    codec.decompress(src, lod=kk)
                    t1 = time.perf_counter()
                    if it:
                        t[kk].append(t1 - t0)
            nbytes = sum(nb for nb, _ in info)
            rows[str(k)] = {"prefix_bytes": nbytes, "share": round(nbytes / total, 4), "cells": sum(m for _, m in info),
                            "ms_per_frame": round(med_ms(t[k]) / B, 4), "ms_k0_beside": round(med_ms(t[0]) / B, 4)}
            print(f"{name} lod={k}", json.dumps(rows[str(k)]), flush=True)
        res["workloads"][name] = {"frames": B, "points": sum(p.shape[0] for p in full), "blob_bytes": total, "lod": rows}
    codec.close()
    if args.only_lod is not None:
        return
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
