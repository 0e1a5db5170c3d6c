#!/usr/bin/env python3
"""Near-lossless attributes: B KITTI-like sweeps with their intensity (workloads.lidar_sweep(seed=s),
workloads.lidar_intensity(seed=s)), B in {1, 8, 32}.  In one process and alternating, ms per sweep (median of REPS):
GeometryCodec.compress(attributes=, max_error=e) and decompress of its blobs for e = 0 (lossless, versions 1 / 2) against
e in {1, 4} (versions 4 / 7), both kinds (scalable False / True).  Host arrays in, host arrays out.  Every timed result
is checked once: no decoded value off by more than e from the lossless result.

Also the bytes and bits per value of the sweep's intensity and of the 1M-point room's RGB for e in {0, 1, 2, 4, 8}.
Writes one JSON object (stdout, and --out).  --calls N: only N compress + decompress calls of B = 1 at --e, both kinds
(for a rocprofv3 --kernel-trace --stats run of its own)."""
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
ES = (0, 1, 4)


def med_ms(v):
    return 1e3 * float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "7")))
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--e", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    codec = pkg.GeometryCodec()
    if args.calls:
        p = wl.lidar_sweep(seed=0)["points"]
        a = wl.lidar_intensity(p, seed=0)
        for _ in range(args.calls):
            for scalable in (False, True):
                g, ab = codec.compress([p], attributes=[a], scalable=scalable, max_error=args.e)
                codec.decompress(g, ab)
        torch.cuda.synchronize()
        codec.close()
        return
    batches = [int(b) for b in args.batches.split(",")]
    sweeps = [wl.lidar_sweep(seed=s)["points"] for s in range(max(batches))]
    inten = [wl.lidar_intensity(p, seed=s) for s, p in enumerate(sweeps)]
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "points_per_sweep": int(np.mean([p.shape[0] for p in sweeps])), "B": {}}
    for B in batches:
        blobs, jobs, sizes = {}, {}, {}
        for scalable in (False, True):
            kind = "scalable" if scalable else "plain"
            exact = None
            for e in ES:
                g, ab = codec.compress(sweeps[:B], attributes=inten[:B], scalable=scalable, max_error=e)
                vals = codec.decompress(g, ab)[1]
                if e == 0:
                    exact = vals
                for x, y in zip(vals, exact):
                    assert np.abs(x.astype(np.int64) - y.astype(np.int64)).max() <= e, (kind, e)
                blobs[kind, e] = (g, ab)
                sizes[f"{kind}_e{e}"] = int(np.mean([len(b) for b in ab]))
                jobs[f"enc_{kind}_e{e}"] = (lambda s, e: lambda: codec.compress(sweeps[:B], attributes=inten[:B], scalable=s,
                                                                                max_error=e))(scalable, e)
                jobs[f"dec_{kind}_e{e}"] = (lambda k: lambda: codec.decompress(*blobs[k]))((kind, e))
        names = list(jobs)
        t = {k: [] for k in names}
        for it in range(args.reps + 1):
            for name in (names if it % 2 == 0 else names[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jobs[name]()
                dt = time.perf_counter() - t0
                if it:
                    t[name].append(dt)
        r = {k: round(med_ms(v) / B, 4) for k, v in t.items()}   # ms per sweep
        r["spread"] = {k: [round(1e3 * min(v) / B, 4), round(1e3 * max(v) / B, 4)] for k, v in t.items()}
        r["attr_bytes_per_sweep"] = sizes
        res["B"][str(B)] = r
        print(f"B={B}", json.dumps(r), flush=True)
    room = wl.room(1_000_000, seed=0)
    rates = {}
    for name, pts, vals in (("sweep_intensity", sweeps[0], inten[0]),
                            ("room_rgb", room["points"], np.rint(255 * room["colors"]).astype(np.uint8))):
        per = {}
        for scalable in (False, True):
            for e in (0, 1, 2, 4, 8):
                ab = codec.compress([pts], attributes=[vals], scalable=scalable, max_error=e)[1][0]
                info = pkg.GeometryCodec.attr_info(ab)
                nv = info["points"] * info["channels"]
                per[f"{'scalable' if scalable else 'plain'}_e{e}"] = {"version": info["version"], "bytes": len(ab),
                                                                     "bits_per_value": round(8 * len(ab) / nv, 4)}
        rates[name] = per
        print(name, json.dumps(per), flush=True)
    res["rates"] = rates
    codec.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
