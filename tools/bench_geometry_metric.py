#!/usr/bin/env python3
"""Metric frames of GeometryCodec: what the float32 front end, device-resident frames, the row index and float32
output cost, in ms per sweep.

Workload (seeded): B = 1 / 8 / 32 KITTI-like sweeps (workloads.lidar_sweep(seed=s)) taken back to metres at the
sweep's voxel (0.02 m) and moved off the lattice by a seeded jitter, float32 [n, 3] per sweep.  Per B, the variants
alternate in one process, the order reversed every round, median of REPS:
  a  host prologue np.rint(p / voxel).astype(np.int16) per frame ("a_prologue"), then today's compress(int16 frames)
     ("a_compress"); "a_total" times both in one span
  b  compress(float32 host frames, voxel=)
  c  compress(float32 device frames, voxel=)
  d  b with return_index=True
  e  decompress to int32 ("e_int32") against decompress(voxel=) to float32 ("e_float32"), host arrays; and both with
     output="device" ("e_int32_dev", "e_float32_dev")
b's blobs are checked against compress of the numpy restatement's lattice (tests/metric_ref.py).  Writes one JSON
object (stdout, --out)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "demo-learned-point-cloud-compression_amd"
VOXEL = 0.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "9")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import metric_ref
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    codec = pkg.GeometryCodec()
    dev = codec.rt.device
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "voxel": VOXEL, "B": {}}
    rng = np.random.default_rng(2026)
    sweeps = {}
    for B in [int(b) for b in args.batches.split(",")]:
        for s in range(B):
            if s not in sweeps:
                p = wl.lidar_sweep(seed=s)["points"].astype(np.float64)
                sweeps[s] = ((p + rng.uniform(-0.45, 0.45, p.shape)) * float(np.float32(VOXEL))).astype(np.float32)
        frames = [sweeps[s] for s in range(B)]
        on_dev = [torch.from_numpy(f).to(dev) for f in frames]
        torch.cuda.synchronize()
        blobs = codec.compress(frames, voxel=VOXEL)
        assert blobs == codec.compress([metric_ref.quantize(f, VOXEL)[0] for f in frames])
        assert blobs == codec.compress(on_dev, voxel=VOXEL)
        state = {}

        def prologue():
            state["q"] = [np.rint(f / VOXEL).astype(np.int16) for f in frames]

        def a_total():
            codec.compress([np.rint(f / VOXEL).astype(np.int16) for f in frames])

        variants = {
            "a_prologue": prologue,
            "a_compress": lambda: codec.compress(state["q"]),
            "a_total": a_total,
            "b_float_host": lambda: codec.compress(frames, voxel=VOXEL),
            "c_float_device": lambda: codec.compress(on_dev, voxel=VOXEL),
            "d_float_host_index": lambda: codec.compress(frames, voxel=VOXEL, return_index=True),
            "e_int32": lambda: codec.decompress(blobs),
            "e_float32": lambda: codec.decompress(blobs, voxel=VOXEL),
            "e_int32_dev": lambda: codec.decompress(blobs, output="device"),
            "e_float32_dev": lambda: codec.decompress(blobs, output="device", voxel=VOXEL),
        }
        names = list(variants)
        t = {k: [] for k in names}
        for it in range(args.reps + 1):      # round 0 warms up
            for k in (names if it % 2 == 0 else names[:1] + names[:0:-1]):      # the prologue stays in front of a_compress
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                variants[k]()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if it:
                    t[k].append(t1 - t0)
        row = {k: round(1e3 * float(np.median(v)) / B, 4) for k, v in t.items()}
        row["points_per_sweep"] = int(sum(f.shape[0] for f in frames) / B)
        res["B"][str(B)] = row
        print(f"B={B}", json.dumps(row), flush=True)
    codec.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
