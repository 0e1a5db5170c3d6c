#!/usr/bin/env python3
"""A byte budget for transform-coded attributes (compress(..., qstep=, target_bytes=)) beside the same search done with
the calls that existed before it.  On the GPU, one process, one library: ms per call (median of REPS, the jobs
alternating, the order reversed every other round; a call ends when its blobs are on the host) of
  (a) budget     the budgeted call;
  (b) host_loop  the search as a host loop of plain compress(..., qstep=steps) calls over exactly the rungs the
                 procedure visits, each call coding the frames that visit that rung (the visits are worked out
                 beforehand, outside the timed window, so the loop pays for the coding alone);
  (c) plain      one compress(..., qstep=qstep) call, no budget.
Inputs (qstep (4, 8, 8) with the colour transform; the target is --share of each frame's length at qstep):
  zed1       recorded frame 0 of tests/golden/zed_seq25.npz, one frame per call
  zed25      the 25 recorded frames, one call
  room_rgb   workloads.room(1M) with its colours, one frame
Before timing, every budgeted blob is checked against the blob of the host loop's choice.  Writes one JSON object
(stdout, and --out)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "demo-learned-point-cloud-compression_amd"
Q = (4, 8, 8)


def timing(reps, share, scratch_limit):
    import torch
    import attr_rate_ref as R
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    G = pkg.GeometryCodec
    codec = G()
    codec.rate_scratch_limit = scratch_limit
    with np.load(os.path.join(ROOT, "tests", "golden", "zed_seq25.npz")) as f:
        zed = [(f[f"points_{i}"].astype(np.int32), f[f"colors_u8_{i}"]) for i in range(int(f["n_frames"]))]
    room = wl.room(1_000_000, seed=0)
    inputs = {"zed1": ([zed[0][0]], [zed[0][1]]),
              "zed25": ([p for p, _ in zed], [a for _, a in zed]),
              "room_rgb": ([room["points"]], [np.rint(255 * room["colors"]).astype(np.uint8)])}
    ladder = G.rate_ladder(Q, np.uint8)
    J = len(ladder)
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "qstep": list(Q), "colour": "ycocg", "share": share,
           "scratch_limit": scratch_limit, "rungs": J, "inputs": {}}
    kw = dict(colour="ycocg")
    for name, (frames, attrs) in inputs.items():
        nf = len(frames)
        at = [codec.compress(frames, attributes=attrs, qstep=s, **kw)[1] for s in ladder]      # the oracle, outside the timed window
        targets = [max(1, int(share * len(at[0][f]))) for f in range(nf)]
        found = [R.choose(lambda j: len(at[j][f]), J, targets[f]) for f in range(nf)]
        visits = {}                                                         # rung -> the frames that visit it
        for f, (_, seen) in enumerate(found):
            for j in seen:
                visits.setdefault(j, []).append(f)
        got = codec.compress(frames, attributes=attrs, qstep=Q, target_bytes=targets, **kw)[1]
        assert all(got[f] == at[found[f][0]][f] for f in range(nf)), name
        calls = [(ladder[j], [frames[f] for f in fs], [attrs[f] for f in fs]) for j, fs in sorted(visits.items())]

        def host_loop():
            for steps, fr, a in calls:
                codec.compress(fr, attributes=a, qstep=steps, **kw)
        jobs = {"budget": lambda: codec.compress(frames, attributes=attrs, qstep=Q, target_bytes=targets, **kw),
                "host_loop": host_loop,
                "plain": lambda: codec.compress(frames, attributes=attrs, qstep=Q, **kw)}
        names = list(jobs)
        t = {k: [] for k in names}
        for it in range(reps + 1):                                          # round 0 warms up
            for job in (names if it % 2 == 0 else names[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jobs[job]()
                dt = time.perf_counter() - t0
                if it:
                    t[job].append(dt)
        rungs = [r for r, _ in found]
        out = {"frames": nf, "points": int(sum(p.shape[0] for p in frames)), "target_bytes": int(sum(targets)),
               "bytes": int(sum(len(b) for b in got)), "bytes_at_qstep": int(sum(len(b) for b in at[0])),
               "rungs_chosen": [min(rungs), max(rungs)], "host_loop_calls": len(calls),
               "host_loop_frame_codings": int(sum(len(fs) for fs in visits.values())),
               "ms_per_call": {k: round(1e3 * float(np.median(v)), 3) for k, v in t.items()},
               "spread": {k: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in t.items()}}
        out["budget_below_host_loop_by_more_than_its_spread"] = bool(
            out["ms_per_call"]["host_loop"] - out["ms_per_call"]["budget"] > out["spread"]["host_loop"][1] - out["spread"]["host_loop"][0])
        res["inputs"][name] = out
        print(name, json.dumps(out), flush=True)
    codec.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "9")))
    ap.add_argument("--share", type=float, default=0.4, help="a frame's target as a share of its length at qstep")
    ap.add_argument("--scratch-limit", type=int, default=0, help="GeometryCodec.rate_scratch_limit, bytes (0: the default)")
    ap.add_argument("--commit", default=None, help="recorded in the result")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"commit": args.commit, "timing": timing(args.reps, args.share, args.scratch_limit)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
