#!/usr/bin/env python3
"""Geometry-only coding of a sequence of B KITTI-like sweeps (workloads.lidar_sweep(seed=s)), B in {1, 8, 32}: a loop
of single-sweep calls against one batched call, in the same process and alternating, ms per sweep (median of REPS).

  codec : GeometryCodec.compress / decompress — host points -> blobs -> host points (upload, keys, sort, unique
          included); loop = one call per sweep, batch = one call for all B
  coder : Morton-sorted keys in HBM -> blobs on the host -> host points: Runtime.octree_encode(version=2) /
          octree_decode per sweep against octree_encode_frames / octree_decode_frames

Every batched blob is checked against the single-sweep blob.  Writes one JSON object (stdout, and --out)."""
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
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "7")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    batches = [int(b) for b in args.batches.split(",")]
    sweeps = [wl.lidar_sweep(seed=s)["points"] for s in range(max(batches))]
    codec = pkg.GeometryCodec()
    rt = codec.rt
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "points_per_sweep": int(np.mean([p.shape[0] for p in sweeps])), "B": {}}
    with rt:
        keys_all = []
        for s, p in enumerate(sweeps):   # one frame per sweep, batch index 0 (single path) and s (batched path)
            k = rt.morton_keys(rt.to_device(np.concatenate([np.zeros((p.shape[0], 1), np.int32), p.astype(np.int32)], 1)))
            rt.sort_pairs(k)
            keys_all.append(k)
        torch.cuda.synchronize()
    for B in batches:
        frames = sweeps[:B]
        with rt:
            bk = torch.cat([k + (s << 48) for s, k in enumerate(keys_all[:B])])
            torch.cuda.synchronize()
        t = {k: [] for k in ("codec_loop_enc", "codec_loop_dec", "codec_batch_enc", "codec_batch_dec",
                             "coder_loop_enc", "coder_loop_dec", "coder_batch_enc", "coder_batch_dec")}
        for it in range(args.reps + 1):
            for order in ((0, 1) if it % 2 == 0 else (1, 0)):
                torch.cuda.synchronize()
                if order == 0:     # loops of single-sweep calls
                    t0 = time.perf_counter()
                    loop = [codec.compress([p])[0] for p in frames]
                    t1 = time.perf_counter()
                    lpts = [codec.decompress([b])[0] for b in loop]
                    t2 = time.perf_counter()
                    with rt:
                        cl = [rt.octree_encode(k, 0, version=2) for k in keys_all[:B]]
                        t3 = time.perf_counter()
                        cp = [rt.octree_decode(b) for b in cl]
                        t4 = time.perf_counter()
                    if it:
                        t["codec_loop_enc"].append(t1 - t0); t["codec_loop_dec"].append(t2 - t1)
                        t["coder_loop_enc"].append(t3 - t2); t["coder_loop_dec"].append(t4 - t3)
                else:              # one batched call
                    t0 = time.perf_counter()
                    batch = codec.compress(frames)
                    t1 = time.perf_counter()
                    bpts = codec.decompress(batch)
                    t2 = time.perf_counter()
                    with rt:
                        cb = rt.octree_encode_frames(bk, B)
                        t3 = time.perf_counter()
                        cbp = rt.octree_decode_frames(cb)
                        t4 = time.perf_counter()
                    if it:
                        t["codec_batch_enc"].append(t1 - t0); t["codec_batch_dec"].append(t2 - t1)
                        t["coder_batch_enc"].append(t3 - t2); t["coder_batch_dec"].append(t4 - t3)
        assert batch == loop == cb == cl, "batched blobs differ from the single-sweep blobs"
        assert all(np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
                   for a, b, c, d in zip(lpts, bpts, cp, cbp))
        r = {k: round(med_ms(v) / B, 4) for k, v in t.items()}   # ms per sweep
        for part in ("codec", "coder"):
            for d in ("enc", "dec"):
                r[f"{part}_{d}_speedup"] = round(r[f"{part}_loop_{d}"] / r[f"{part}_batch_{d}"], 2)
        r["blob_bytes_per_sweep"] = int(np.mean([len(b) for b in batch]))
        res["B"][str(B)] = r
        print(f"B={B}", json.dumps(r), flush=True)
    codec.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
