#!/usr/bin/env python3
"""Attributes at a level of detail: B KITTI-like sweeps with their intensity (workloads.lidar_sweep(seed=s),
workloads.lidar_intensity(seed=s)), B in {1, 8, 32}.  In one process and alternating, ms per sweep (median of REPS):
GeometryCodec.compress(attributes=) writing attribute blob version 1 against scalable=True (version 2), and
decompress of version 1, of version 2 at lod 0 and of the two shortest prefixes (geometry and attributes) at lod 1 .. 4.
Host arrays in, host arrays out.  Every timed result is checked once against the others (version 2 at lod 0 equals
version 1; a level's rows equal the values of the Morton-first points).

Also bytes and values per lod of the sweep's intensity and of the 1M-point room's RGB, and bits per value of version 2
beside version 1.  Writes one JSON object (stdout, and --out).  --calls N: only N compress(scalable=True) + decompress
calls at --lod of B = 1 (for a rocprofv3 --kernel-trace --stats run of its own)."""
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
LODS = (1, 2, 3, 4)


def med_ms(v):
    return 1e3 * float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "7")))
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--lod", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    GeometryCodec = pkg.GeometryCodec
    codec = GeometryCodec()
    if args.calls:
        p = wl.lidar_sweep(seed=0)["points"]
        a = wl.lidar_intensity(p, seed=0)
        for _ in range(args.calls):
            g, ab = codec.compress([p], attributes=[a], scalable=True)
            codec.decompress([g[0][:GeometryCodec.lod_info(g[0], args.lod)[0]]],
                             [ab[0][:GeometryCodec.attr_lod_info(ab[0], args.lod)[0]]], lod=args.lod)
        torch.cuda.synchronize()
        codec.close()
        return
    import attr2_ref
    batches = [int(b) for b in args.batches.split(",")]
    sweeps = [wl.lidar_sweep(seed=s)["points"] for s in range(max(batches))]
    inten = [wl.lidar_intensity(p, seed=s) for s, p in enumerate(sweeps)]
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "points_per_sweep": int(np.mean([p.shape[0] for p in sweeps])), "B": {}}
    for B in batches:
        g, a1 = codec.compress(sweeps[:B], attributes=inten[:B])
        g2, a2 = codec.compress(sweeps[:B], attributes=inten[:B], scalable=True)
        assert g == g2
        pre = {k: ([b[:GeometryCodec.lod_info(b, k)[0]] for b in g], [b[:GeometryCodec.attr_lod_info(b, k)[0]] for b in a2])
               for k in LODS}
        full_p, full_v = codec.decompress(g, a1)
        for x, y in zip(codec.decompress(g, a2)[1], full_v):
            assert np.array_equal(x, y)
        for k in LODS:      # a level's rows: the values of the Morton-first points of its cells
            cells, vals = codec.decompress(*pre[k], lod=k)
            _, idx = np.unique(attr2_ref.keys_of(full_p[0] >> k, 32768 >> k), return_index=True)
            assert np.array_equal(cells[0], full_p[0][idx] >> k) and np.array_equal(vals[0], full_v[0][idx]), k
        names = ["enc_v1", "enc_v2", "dec_v1", "dec_v2_lod0"] + [f"dec_v2_lod{k}" for k in LODS]
        jobs = {"enc_v1": lambda: codec.compress(sweeps[:B], attributes=inten[:B]),
                "enc_v2": lambda: codec.compress(sweeps[:B], attributes=inten[:B], scalable=True),
                "dec_v1": lambda: codec.decompress(g, a1),
                "dec_v2_lod0": lambda: codec.decompress(g, a2)}
        for k in LODS:
            jobs[f"dec_v2_lod{k}"] = (lambda k: lambda: codec.decompress(*pre[k], lod=k))(k)
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
        r["attr_bytes_per_sweep"] = {"v1": int(np.mean([len(b) for b in a1])), "v2": int(np.mean([len(b) for b in a2]))}
        for k in LODS:
            r["attr_bytes_per_sweep"][f"v2_lod{k}"] = int(np.mean([len(b) for b in pre[k][1]]))
        res["B"][str(B)] = r
        print(f"B={B}", json.dumps(r), flush=True)
    room = wl.room(1_000_000, seed=0)
    levels = {}
    for name, pts, vals in (("sweep_intensity", sweeps[0], inten[0]),
                            ("room_rgb", room["points"], np.rint(255 * room["colors"]).astype(np.uint8))):
        g, a1 = codec.compress([pts], attributes=[vals])
        _, a2 = codec.compress([pts], attributes=[vals], scalable=True)
        n = GeometryCodec.attr_lod_info(a2[0], 0)[1]
        nv = n * (1 if vals.ndim == 1 else vals.shape[1])
        per = []
        for k in range(0, 7):
            ab, av = GeometryCodec.attr_lod_info(a2[0], k)
            gb, gv = GeometryCodec.lod_info(g[0], k)
            assert av == gv
            per.append({"lod": k, "values": av, "attr_bytes": ab, "attr_share": round(ab / len(a2[0]), 4),
                        "geometry_bytes": gb, "geometry_share": round(gb / len(g[0]), 4)})
        levels[name] = {"points": n, "bits_per_value": {"v1": round(8 * len(a1[0]) / nv, 4), "v2": round(8 * len(a2[0]) / nv, 4)},
                        "bytes": {"v1": len(a1[0]), "v2": len(a2[0])}, "v2_excess": round(len(a2[0]) / len(a1[0]) - 1, 5),
                        "levels": per}
        print(name, json.dumps(levels[name]), flush=True)
    res["levels"] = levels
    codec.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
