#!/usr/bin/env python3
"""Cross-channel attribute blobs (versions 8, 11, 13, 14) against the plain kinds (1, 2, 4, 7) of the same build: bytes,
and ms per call (median of REPS) of GeometryCodec.compress(attributes=, cross_channel=) and of decompress of its blobs,
plain and cross alternating in one process.  Host arrays in, host arrays out.  Inputs:
  zed25      the 25 recorded camera frames of tests/golden/zed_seq25.npz with their RGB, one call
  room_rgb   workloads.room(1M) with its colours, one frame
  intensity  workloads.lidar_sweep + lidar_intensity: one channel, so the cross call must give the plain bytes
Kinds: lossless and max_error = --e, unscalable and scalable.  Every timed result is checked once: the cross call decodes
to exactly what the plain call decodes to.  Also the per-frame bytes of recorded frames 0 and 20 for e in {0, 1, 2, 4}.
Writes one JSON object (stdout, and --out)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "7")))
    ap.add_argument("--e", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    codec = pkg.GeometryCodec()
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        zed = [(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"]) for i in range(int(f["n_frames"]))]
    room = wl.room(1_000_000, seed=0)
    sweep = wl.lidar_sweep(seed=0)["points"]
    inputs = {"zed25": ([p for p, _ in zed], [a for _, a in zed]),
              "room_rgb": ([room["points"]], [np.rint(255 * room["colors"]).astype(np.uint8)]),
              "intensity": ([sweep], [wl.lidar_intensity(sweep, seed=0)])}
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "e": args.e, "inputs": {}}
    for name, (frames, attrs) in inputs.items():
        blobs, jobs, out = {}, {}, {"frames": len(frames), "points": int(sum(p.shape[0] for p in frames)), "kinds": {}}
        for scalable in (False, True):
            for e in (0, args.e):
                kw = dict(scalable=scalable, max_error=e)
                exact = None
                for cross in (False, True):
                    g, ab = codec.compress(frames, attributes=attrs, cross_channel=cross, **kw)
                    vals = codec.decompress(g, ab)[1]
                    if not cross:
                        exact, plain_ab = vals, ab
                    assert all(np.array_equal(x, y) for x, y in zip(vals, exact)), (name, kw)
                    key = f"v{ab[0][1]}"
                    blobs[key] = (g, ab)
                    out["kinds"][key] = {"bytes": int(sum(len(b) for b in ab)), "geometry_bytes": int(sum(len(b) for b in g))}
                    if cross:
                        out["kinds"][key]["of_plain"] = round(sum(len(b) for b in ab) / sum(len(b) for b in plain_ab), 4)
                        out["kinds"][key]["same_bytes_as_plain"] = ab == plain_ab
                    tag = f"{key}{'x' if cross and ab == plain_ab else ''}"
                    jobs[f"enc_{tag}"] = (lambda c, k: lambda: codec.compress(frames, attributes=attrs, cross_channel=c, **k))(cross, kw)
                    jobs[f"dec_{tag}"] = (lambda k: lambda: codec.decompress(*blobs[k]))(key)
        names = list(jobs)
        t = {k: [] for k in names}
        for it in range(args.reps + 1):
            for job in (names if it % 2 == 0 else names[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jobs[job]()
                dt = time.perf_counter() - t0
                if it:
                    t[job].append(dt)
        out["ms_per_call"] = {k: round(med_ms(v), 3) for k, v in t.items()}
        out["spread"] = {k: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in t.items()}
        res["inputs"][name] = out
        print(name, json.dumps(out), flush=True)
    table = {}
    for i in (0, 20):
        p, a = zed[i]
        per = {}
        for scalable in (False, True):
            for e in (0, 1, 2, 4):
                plain = codec.compress([p], attributes=[a], scalable=scalable, max_error=e)[1][0]
                cross = codec.compress([p], attributes=[a], scalable=scalable, max_error=e, cross_channel=True)[1][0]
                per[f"v{cross[1]}_e{e}"] = {"plain": len(plain), "cross": len(cross), "ratio": round(len(cross) / len(plain), 4)}
        table[f"frame_{i}"] = per
        print(f"frame {i}", json.dumps(per), flush=True)
    res["recorded_frames"] = table
    codec.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
