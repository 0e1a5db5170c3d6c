#!/usr/bin/env python3
"""compress(..., predict="best") on one MI355X (pcc_octree_encode_frames_inter_best; include/pcc.h has the rule): what
choosing per frame between version 2 and a window saves, and what coding every candidate costs.

Inputs: workloads.lidar_sequence(10, 64, 1800) with the sensor at rest and at 10 m/s, and the 25 recorded camera frames
of tests/golden/zed_seq25.npz.  Per input, in one process:
  bytes   per frame and in total of predict=None, predict="previous" with K = 1 and K = 4, and predict="best" with
          K = 4, and how often each candidate (version 2, W = 1 .. 4) won;
  times   median wall milliseconds per frame of an encode call, Morton-sorted keys in HBM to blobs on the host, of
          "best" K = 4, of "previous" K = 4, and of the five separate calls that produce the candidates of "best"
          (version 2, and windows of up to 1, 2, 3 and 4 frames) in sum — the three measured in turn, round after
          round, behind WARMUP (3) rounds that are not counted, REPS (15) rounds; the spread is min .. max.
One JSON line per input, also written to profiles/geometry_inter_best.json (--out: elsewhere).  The blobs of "best" are
checked: every one is the shortest of the five calls' blobs of its frame that the rule lets it take, and the sequence
decodes to the frames."""
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
K = 4


def rounds(calls, warmup, reps):
    """{name: [wall ms of each counted round]}: the calls in turn, round after round, each behind a device synchronise"""
    t = {name: [] for name in calls}
    for it in range(warmup + reps):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                t[name].append(1e3 * (time.perf_counter() - t0))
    return t


def measure(rt, name, frames, warmup, reps):
    n = len(frames)
    coords = np.concatenate([np.concatenate([np.full((p.shape[0], 1), f, np.int32), p], 1) for f, p in enumerate(frames)])
    keys = rt.morton_keys(rt.to_device(coords))
    rt.sort_pairs(keys)
    v2 = rt.octree_encode_frames(keys, n)
    prev = {1: rt.octree_encode_frames_inter(keys, n)}
    for k in range(2, K + 1):
        prev[k] = rt.octree_encode_frames_inter_hist(keys, n, history=k)
    best = rt.octree_encode_frames_inter_best(keys, n, history=K)
    # every blob of "best" is one of the five calls' blobs of its frame, and the shortest the rule lets it take
    wins = {"v2": 0, **{"W%d" % w: 0 for w in range(1, K + 1)}}
    for f in range(n):
        cands = [(0, v2[f])] + [(w, prev[w][f]) for w in range(1, min(f, K) + 1)]      # previous K = w gives frame f >= w a window of w
        w, want = min(cands, key=lambda c: (len(c[1]), c[0]))
        assert best[f] == want, (name, f, w, len(best[f]), len(want))
        wins["v2" if w == 0 else "W%d" % w] += 1
    got = rt.octree_decode_frames_refs(best)
    want = rt.octree_decode_frames(v2)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))

    def five():
        rt.octree_encode_frames(keys, n)
        rt.octree_encode_frames_inter(keys, n)
        for k in range(2, K + 1):
            rt.octree_encode_frames_inter_hist(keys, n, history=k)
    t = rounds({"best": lambda: rt.octree_encode_frames_inter_best(keys, n, history=K),
                "previous": lambda: rt.octree_encode_frames_inter_hist(keys, n, history=K),
                "five_calls": five}, warmup, reps)
    calls = {"none": v2, "previous_K1": prev[1], "previous_K4": prev[K], "best_K4": best}
    res = {"input": name, "frames": n, "points": [int(p.shape[0]) for p in frames],
           "bytes_per_frame": {c: [len(b) for b in blobs] for c, blobs in calls.items()},
           "bytes_total": {c: sum(len(b) for b in blobs) for c, blobs in calls.items()},
           "wins_of_best_K4": wins, "warmup_rounds": warmup, "rounds": reps,
           "encode_ms_per_frame": {c: {"median": float(np.median(v)) / n, "min": min(v) / n, "max": max(v) / n} for c, v in t.items()}}
    res["bytes_ratio_to_none"] = {c: res["bytes_total"][c] / res["bytes_total"]["none"] for c in calls}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_inter_best.json"))
    args = ap.parse_args()
    importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    rtm = importlib.import_module(PKG + ".runtime")
    warmup, reps = int(os.environ.get("WARMUP", "3")), int(os.environ.get("REPS", "15"))
    inputs = [("lidar_sequence(10, 64, 1800) at rest", [f["points"].astype(np.int32) for f in wl.lidar_sequence(10, 64, 1800)]),
              ("lidar_sequence(10, 64, 1800) at 10 m/s",
               [f["points"].astype(np.int32) for f in wl.lidar_sequence(10, 64, 1800, velocity=(10, 0, 0))])]
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        inputs.append(("zed_seq25.npz, 25 recorded frames", [np.unique(f[f"points_{i}"].astype(np.int32), axis=0) for i in range(25)]))
    rt = rtm.Runtime(0)
    lines = []
    with rt:
        for name, frames in inputs:
            lines.append(json.dumps(measure(rt, name, frames, warmup, reps)))
            print(lines[-1], flush=True)
    rt.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
