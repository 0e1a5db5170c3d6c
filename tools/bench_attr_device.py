#!/usr/bin/env python3
"""Device-resident and float attributes into GeometryCodec (csrc/attr_stage.hip): ms per call of compress and transfer
with the attributes on the host, on the device, and on the device but taken through .cpu().numpy() first — what a
caller with device-resident attributes had to do before the codec read them where they lie.

Inputs (seeded):
  room     workloads.room(1_000_000) with its RGB as uint8, one frame
  zed      the eight recorded camera frames of tests/golden/zed_seq25.npz with their RGB, one call of eight frames
  voxel    a synthetic camera frame through capture.voxelize(output="device"): int32 points and float64 colours in
           [0, 1] on the device, coded with attribute_scale=255 (the .cpu() route quantises them on the host)
transfer carries the attributes onto the centres of the frames' lod-1 cells.  Frames are where the attributes are.

Median of 10 calls behind 2 warm-ups, the variants taking turns in one process; beside each median the range.  Beside
each input: the bytes the staging kernel moves in packed mode (values read, values written) and what a plain device copy
of that many bytes takes (tools/hbm_copy.py's method).

--host-only: the host-attribute calls alone, with a sha256 over their blobs and results — runs on any commit that has
GeometryCodec.transfer, so --root <checkout> measures a parent's build with this file.
--calls N: only N device-attribute calls per input, for a rocprofv3 --kernel-trace --stats run of its own;
--kernel-trace <csv> reads that run's k_attr_stage dispatches back.  Writes one JSON object (stdout, --out)."""
import argparse
import csv
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

PKG = "demo-learned-point-cloud-compression_amd"
CASES = ("room", "zed", "voxel")


def camera_frame(seed=7, w=320, h=240):
    """XYZRGBA float32 [w h, 4]: a wall and a floor seen from the origin, random colours"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(-0.6, 0.6, w), np.linspace(-0.45, 0.45, h))
    d = np.stack([u, v, -np.ones_like(u)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = np.full(d.shape[0], 1.2)
    t = np.where(d[:, 1] < -0.05, np.minimum(t, -0.35 / np.minimum(d[:, 1], -1e-6)), t)
    p = (d * t[:, None] + rng.normal(0, 0.0008, d.shape)).astype(np.float32)
    rgba = (rng.integers(0, 256, d.shape[0], dtype=np.uint32) | (rng.integers(0, 256, d.shape[0], dtype=np.uint32) << 8)
            | (rng.integers(0, 256, d.shape[0], dtype=np.uint32) << 16) | (np.uint32(255) << 24))
    return np.concatenate([p, rgba.view(np.float32)[:, None]], 1).astype(np.float32)


def inputs(pkg, codec, case, root):
    """(host frames int32, host attributes uint8, device attributes as a caller holds them, the scale or None)"""
    wl = importlib.import_module(PKG + ".workloads")
    dev = codec.rt.device
    if case == "room":
        fr = wl.room(1_000_000)
        frames, attrs = [fr["points"].astype(np.int32)], [np.rint(fr["colors"] * 255.0).astype(np.uint8)]
    elif case == "zed":
        with np.load(os.path.join(root, "tests", "golden", "zed_seq25.npz")) as f:
            frames = [f[f"points_{i}"].astype(np.int32) for i in range(8)]
            attrs = [np.ascontiguousarray(f[f"colors_u8_{i}"]) for i in range(8)]
    else:
        capture = importlib.import_module(PKG + ".capture")
        with codec.rt as rt:
            out = capture.voxelize(rt, camera_frame(), 1.4, 0.005, output="device")
            rt.sync()
        colours = out["colors"]      # float64 [n, 3] in [0, 1]
        points = np.ascontiguousarray(out["points"].cpu().numpy(), dtype=np.int32)
        return [points], [np.rint(colours.cpu().numpy() * 255.0).astype(np.uint8)], [colours], 255
    return frames, attrs, [torch.from_numpy(a).to(dev) for a in attrs], None


def centres(codec, frames, k=1):
    cells = codec.decompress(codec.compress(frames), lod=k)
    return [((c << k) + ((1 << k) >> 1)).astype(np.int32) for c in cells]


def timed(variants, reps=10, warmups=2):
    """{name: call} -> {name: {"median_ms", "min_ms", "max_ms"}}: the variants take turns, call after call"""
    t = {name: [] for name in variants}
    for it in range(warmups + reps):
        for name, call in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if it >= warmups:
                t[name].append(1e3 * (time.perf_counter() - t0))
    return {name: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            for name, v in t.items()}


def plain_copy_ms(nbytes):
    n = max(nbytes // 8, 1)      # n float32 read, n written
    x = torch.empty(n, dtype=torch.float32, device="cuda").normal_()
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        y.copy_(x)
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / 20, 5)


def digest(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def trace_ms(path, cases, calls):
    """per input the median device time in ms of k_attr_stage: every device-attribute call dispatches it once (compress:
    packed; transfer: sorted), compress first"""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if "k_attr_stage" in r["Kernel_Name"]]
    assert len(ms) == 2 * calls * len(cases), len(ms)
    out = {}
    for i, case in enumerate(cases):
        mine = ms[2 * calls * i:2 * calls * (i + 1)]
        out[case] = {"packed_ms": round(float(np.median(mine[:calls])), 5), "sorted_ms": round(float(np.median(mine[calls:])), 5)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all"] + list(CASES))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose package is measured (default: this file's)")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-calls", type=int, default=5, help="the --calls of the run that wrote --kernel-trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    pkg = importlib.import_module(PKG)
    codec = pkg.GeometryCodec()
    dev = codec.rt.device
    cases = CASES if args.case == "all" else (args.case,)
    res = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmups": 2, "root": os.path.basename(root)}
    for case in cases:
        frames, attrs, d_attrs, scale = inputs(pkg, codec, case, root)
        targets = centres(codec, frames)
        kw = {} if scale is None else {"attribute_scale": scale}
        d_frames = [torch.from_numpy(p).to(dev) for p in frames]
        d_targets = [torch.from_numpy(p).to(dev) for p in targets]
        torch.cuda.synchronize()
        if args.calls:
            for _ in range(args.calls):
                codec.compress(d_frames, attributes=d_attrs, **kw)
            for _ in range(args.calls):
                codec.transfer(d_frames, d_attrs, d_targets, output="device", **kw)
            continue
        blobs, attr_blobs = codec.compress(frames, attributes=attrs)
        moved = codec.transfer(frames, attrs, targets)
        n = int(sum(p.shape[0] for p in frames))
        row = {"frames": len(frames), "rows": n, "targets": int(sum(p.shape[0] for p in targets)),
               "attr_blob_bytes": int(sum(len(b) for b in attr_blobs)), "host_sha256": digest(blobs + attr_blobs + moved)}
        variants = {"compress_host": lambda: codec.compress(frames, attributes=attrs),
                    "transfer_host": lambda: codec.transfer(frames, attrs, targets)}
        if not args.host_only:
            def through_cpu():
                host = [a.cpu().numpy() for a in d_attrs]
                return host if scale is None else [np.rint(a * float(scale)).astype(np.uint8) for a in host]
            got = codec.compress(d_frames, attributes=d_attrs, **kw)
            assert got == (blobs, attr_blobs), "device attributes gave other blobs"
            variants.update({
                "compress_device": lambda: codec.compress(d_frames, attributes=d_attrs, **kw),
                "compress_device_through_cpu": lambda: codec.compress(d_frames, attributes=through_cpu()),
                "transfer_device": lambda: codec.transfer(d_frames, d_attrs, d_targets, output="device", **kw),
                "transfer_device_through_cpu": lambda: codec.transfer(d_frames, through_cpu(), d_targets, output="device")})
            src_b = int(sum(a.numel() * a.element_size() for a in d_attrs))
            row["stage_bytes_packed"] = src_b + int(sum(a.nbytes for a in attrs))
            row["plain_copy_same_bytes_ms"] = plain_copy_ms(row["stage_bytes_packed"])
        row.update(timed(variants))
        res[case] = row
        print(case, json.dumps(row), flush=True)
    codec.close()
    if args.calls:
        return
    if args.kernel_trace:
        for case, k in trace_ms(args.kernel_trace, cases, args.trace_calls).items():
            res[case]["kernel"] = k
            res[case]["packed_gb_per_s"] = round(res[case]["stage_bytes_packed"] / k["packed_ms"] / 1e6, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
