#!/usr/bin/env python3
"""Geometry plus per-point intensity of B KITTI-like sweeps (workloads.lidar_sweep(seed=s) with
workloads.lidar_intensity(seed=s)), B in {1, 8, 32}: GeometryCodec.compress / decompress of the sweeps alone against the
same call with attributes=, in the same process and alternating, ms per sweep (median of REPS).  Host arrays in, host
arrays out (upload, keys, sort and unique included in both).

Also bits per value of the sweep's intensity and of the 1M-point room's RGB (rint(255 colors)) in Morton order: raw,
zlib 9, lzma 9, the attribute blob, and the restatement's single-stream form (tests/attr_ref.py; one lane over the whole
frame).  Writes one JSON object (stdout, and --out).  --calls N: only N compress + decompress calls of B = 1 (for a
rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import importlib
import json
import lzma
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "demo-learned-point-cloud-compression_amd"


def med_ms(v):
    return 1e3 * float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "7")))
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    codec = pkg.GeometryCodec()
    if args.calls:
        p = wl.lidar_sweep(seed=0)["points"]
        a = wl.lidar_intensity(p, seed=0)
        for _ in range(args.calls):
            blobs, ab = codec.compress([p], attributes=[a])
            codec.decompress(blobs, ab)
        torch.cuda.synchronize()
        codec.close()
        return
    batches = [int(b) for b in args.batches.split(",")]
    sweeps = [wl.lidar_sweep(seed=s)["points"] for s in range(max(batches))]
    inten = [wl.lidar_intensity(p, seed=s) for s, p in enumerate(sweeps)]
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "points_per_sweep": int(np.mean([p.shape[0] for p in sweeps])), "B": {}}
    for B in batches:
        t = {k: [] for k in ("geo_enc", "geo_dec", "attr_enc", "attr_dec")}
        for it in range(args.reps + 1):
            for order in ((0, 1) if it % 2 == 0 else (1, 0)):
                torch.cuda.synchronize()
                if order == 0:
                    t0 = time.perf_counter()
                    g = codec.compress(sweeps[:B])
                    t1 = time.perf_counter()
                    codec.decompress(g)
                    t2 = time.perf_counter()
                    k = "geo"
                else:
                    t0 = time.perf_counter()
                    g2, ab = codec.compress(sweeps[:B], attributes=inten[:B])
                    t1 = time.perf_counter()
                    _, vals = codec.decompress(g2, ab)
                    t2 = time.perf_counter()
                    k = "attr"
                if it:
                    t[k + "_enc"].append(t1 - t0)
                    t[k + "_dec"].append(t2 - t1)
        assert g == g2
        r = {k: round(med_ms(v) / B, 4) for k, v in t.items()}   # ms per sweep
        r["intensity_added_enc_ms"] = round(r["attr_enc"] - r["geo_enc"], 4)
        r["intensity_added_dec_ms"] = round(r["attr_dec"] - r["geo_dec"], 4)
        r["geometry_bytes_per_sweep"] = int(np.mean([len(b) for b in g]))
        r["intensity_bytes_per_sweep"] = int(np.mean([len(b) for b in ab]))
        res["B"][str(B)] = r
        print(f"B={B}", json.dumps(r), flush=True)
    # bits per value
    import attr_ref
    room = wl.room(1_000_000, seed=0)
    rates = {}
    for name, pts, vals in (("sweep_intensity", sweeps[0], inten[0]),
                            ("room_rgb", room["points"], np.rint(255 * room["colors"]).astype(np.uint8))):
        g, ab = codec.compress([pts], attributes=[vals])
        _, dec = codec.decompress(g, ab)
        v = dec[0]
        raw = v.tobytes()
        nv = v.size
        S, nc = attr_ref.layout(v.shape[0], v.shape[1])
        rates[name] = {"points": int(v.shape[0]), "channels": int(v.shape[1]), "S": S, "chunks": nc,
                       "bits_per_value": {"raw": 8.0, "zlib9": round(8 * len(zlib.compress(raw, 9)) / nv, 4),
                                          "lzma9": round(8 * len(lzma.compress(raw, preset=9)) / nv, 4),
                                          "blob": round(8 * len(ab[0]) / nv, 4),
                                          "single_stream": round(8 * attr_ref.single_stream_bytes(v, 1) / nv, 4)}}
        print(name, json.dumps(rates[name]), flush=True)
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
