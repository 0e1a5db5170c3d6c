#!/usr/bin/env python3
"""Per call of the geometry coder in a `rocprofv3 --kernel-trace` CSV (run_kernel_trace.csv).

An encode call runs from its first kernel — k_of_check for pcc_octree_encode_frames, the first level kernel
(k_octw_hist / k_oct_frames) for the one-frame path — to its k_o2_pack; a decode call from k_o2_dec to k_o2_points.
Calls are grouped by the coder's grid (the chunks of the call).  Each group reports the number of launches (kernels and
copies / fills) per call, the median GPU-busy time and the median time from the first to the last launch.

    python tools/octree_trace_calls.py run_kernel_trace.csv [summary.json]
"""
import collections
import csv
import json
import statistics
import sys

ENCODE_FIRST_LEVEL_KERNELS = ("k_octw_hist", "k_oct_frames")


def short_name(name):
    """'(anonymous namespace)::k_o2_enc(unsigned char const*, ...)' -> 'k_o2_enc'"""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0].split("<")[0]


def blocks(row):
    return int(row["Grid_Size_X"]) // int(row["Workgroup_Size_X"])


def duration_us(row):
    return (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3


def find(names, start, target):
    """index of the first `target` at or behind `start`, or None"""
    for j in range(start, len(names)):
        if names[j] == target:
            return j
    return None


def call_record(rows, names, i, j):
    segment = rows[i:j + 1]
    return {
        "launches": j - i + 1,
        "busy_us": sum(duration_us(r) for r in segment),
        "span_us": (int(rows[j]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1e3,
        "names": names[i:j + 1],
    }


def split_calls(rows):
    names = [short_name(r["Kernel_Name"]) for r in rows]
    encode = collections.defaultdict(list)   # (path, k_o2_enc blocks) -> calls
    decode = collections.defaultdict(list)   # k_o2_dec blocks -> calls
    i = 0
    while i < len(rows):
        name = names[i]
        batched = name == "k_of_check"
        one_frame = name in ENCODE_FIRST_LEVEL_KERNELS and (i == 0 or names[i - 1] != "k_of_frames")
        if batched or one_frame:
            j = find(names, i, "k_o2_pack")
            if j is None:
                break
            coder = [blocks(r) for r, m in zip(rows[i:j + 1], names[i:j + 1]) if m == "k_o2_enc"]
            if coder:
                encode[("batched" if batched else "one-frame", coder[0])].append(call_record(rows, names, i, j))
            i = j + 1
        elif name == "k_o2_dec":
            j = find(names, i, "k_o2_points")
            if j is None:
                break
            decode[blocks(rows[i])].append(call_record(rows, names, i, j))
            i = j + 1
        else:
            i += 1
    return encode, decode


def summary(calls):
    return {
        "calls": len(calls),
        "launches_per_call": sorted({c["launches"] for c in calls}),
        "gpu_busy_us_median": round(statistics.median(c["busy_us"] for c in calls), 1),
        "first_to_last_launch_us_median": round(statistics.median(c["span_us"] for c in calls), 1),
        "launches": calls[0]["names"],
    }


def main():
    with open(sys.argv[1]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    encode, decode = split_calls(rows)
    out = {"encode": [], "decode": []}
    for (path, coder_blocks), calls in sorted(encode.items()):
        out["encode"].append({"path": path, "k_o2_enc_blocks": coder_blocks, **summary(calls)})
    for coder_blocks, calls in sorted(decode.items()):
        out["decode"].append({"k_o2_dec_blocks": coder_blocks, **summary(calls)})
    for kind in ("encode", "decode"):
        for entry in out[kind]:
            print(kind, {k: v for k, v in entry.items() if k != "launches"})
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
