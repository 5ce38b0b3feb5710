#!/usr/bin/env python3
"""Packed texts (bit planes) against the byte text, on the GPU: python tools/packed_probe.py [--out profiles/packed/packed_text.json]

The driver runs three steps, each a child process under its own `timeout`, and stops at the first that fails:
  1. `measure`  one process: per (text, m) cell the symbols per second of psearch and of the byte text's own path
                (smart_amd.search under the plan's choice for so, bndm and hor; best median of the three), the two
                alternating, REPS repetitions of BATCH back-to-back searches between device events; the streaming-read
                rate over the planes (the plane roofline); the time of planes_pack;
  2. `rocprofv3 --kernel-trace --stats -- ... workload`   kernel times of planes_scan / planes_pack;
  3. `rocprofv3 --pmc FETCH_SIZE -- ... workload`         counters only: what planes_scan fetches against what a plain
                read of the same planes (probe_read) fetches.
One JSON file out.  Times of the packed path: the library's stream events around one psearch_batch of BATCH copies of the
pattern (its host work between the events is a few microseconds); of the byte path: the sum of search_batch's per-pattern
device events."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = (2, 4, 8, 16, 32, 64, 256, 4096)
BATCH, REPS = 20, 5
TEXTS = (("rand4_1Gi", 4, 1 << 30), ("rand2_1Gi", 2, 1 << 30), ("rand4_8Gi", 4, 8 << 30))
BYTE_ALGOS = ("so", "bndm", "hor")


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def measure(out):
    import smart_amd
    from smart_amd import engine
    res = {"batch": BATCH, "reps": REPS, "unit": "symbols per second", "cells": [], "texts": {}}
    for name, sigma, n in TEXTS:
        text = smart_amd.Text.generate(0x5EED0400 + sigma, sigma, n)
        t0 = time.perf_counter()
        pt = smart_amd.PackedText.pack(text)
        pack_ms = [(time.perf_counter() - t0) * 1e3]
        for _ in range(2):  # again, warm: allocation + zero fill + planes_pack + synchronisation, wall clock
            pt.free()
            t0 = time.perf_counter()
            pt = smart_amd.PackedText.pack(text)
            pack_ms.append((time.perf_counter() - t0) * 1e3)
        info = {"sigma": sigma, "symbols": n, "byte_text_bytes": n, "plane_bytes": pt.nbytes, "planes": pt.planes,
                "pack_wall_ms": pack_ms, "pack_wall_ms_per_GiB_of_bytes": min(pack_ms) / (n / 2**30),
                "plane_read_GBps": [pt.probe_read_gbs(20) for _ in range(3)],
                "byte_read_GBps": [engine.probe_read_gbs(text, 20) for _ in range(3)]}
        res["texts"][name] = info
        for m in MS:
            P = text.read(n // 3 + 17, m)
            pats = [P] * BATCH
            want = smart_amd.search("so", P, text)[0]
            packed, packed_wall, byte = [], [], {a: [] for a in BYTE_ALGOS}
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                engine.stream_mark(0, 0)
                counts, wall_ms = smart_amd.psearch_batch(pats, pt)
                engine.stream_mark(0, 1)
                ms = engine.stream_elapsed_ms(0)
                assert counts.tolist() == [want] * BATCH, (name, m, counts.tolist()[:3], want)
                if rep:
                    packed.append(n * BATCH / (ms * 1e-3))
                    packed_wall.append(n * BATCH / (wall_ms * 1e-3))  # first launch to the counts on the host
                for a in BYTE_ALGOS:
                    c, _, run_ms, _ = smart_amd.search_batch(a, pats, text, each=True)
                    assert c.tolist() == [want] * BATCH, (name, a, m)
                    if rep:
                        byte[a].append(n * BATCH / (float(run_ms.sum()) * 1e-3))
            best = max(BYTE_ALGOS, key=lambda a: statistics.median(byte[a]))
            p, b = spread(packed), spread(byte[best])
            gain = p["median"] - b["median"]
            cell = {"text": name, "m": m, "count": want, "packed": p, "packed_by_wall_clock": spread(packed_wall), "byte_best_algo": best, "byte_best": b,
                    "byte_kernel": smart_amd.kernel_for(best, P), "byte_all": {a: spread(byte[a]) for a in BYTE_ALGOS},
                    "ratio_of_medians": p["median"] / b["median"],
                    "speedup": bool(gain > max(p["max"] - p["min"], b["max"] - b["min"])),
                    "share_of_plane_roofline": p["median"] / (statistics.median(info["plane_read_GBps"]) * 1e9 * n / pt.nbytes)}
            res["cells"].append(cell)
            print("%-10s m=%-5d packed %.3e  byte(%s) %.3e  x%.2f  speedup=%s  plane-roofline share %.2f" % (
                name, m, p["median"], best, b["median"], cell["ratio_of_medians"], cell["speedup"], cell["share_of_plane_roofline"]), flush=True)
        pt.free()
        text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload():
    """What the profiler runs look at: 1 GiB of rand4 and of rand2, packed; a plain read of the planes; a few searches."""
    import smart_amd
    for sigma in (4, 2):
        text = smart_amd.Text.generate(0x5EED0400 + sigma, sigma, 1 << 30)
        with smart_amd.PackedText.pack(text) as pt:
            pt.probe_read_gbs(4)
            for m in (8, 32, 256):
                P = text.read((1 << 30) // 3 + 17, m)
                for _ in range(4):
                    smart_amd.psearch(P, pt)
        text.free()


def rows_of(d, suffix):
    for f in sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                yield r


def short(kernel):
    k = kernel.split("(")[0]
    return k[k.index("sg::"):] if "sg::" in k else k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_text.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "packed_probe"))
    a = ap.parse_args()
    a.out, a.scratch = os.path.abspath(a.out), os.path.abspath(a.scratch)
    if a.step == "measure":
        return measure(a.out)
    if a.step == "workload":
        return workload()
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, pmc_dir = os.path.join(a.scratch, "trace"), os.path.join(a.scratch, "pmc")
    steps = [
        ("measure", ["timeout", "-k", "10", "900"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload"]),
        ("FETCH_SIZE", ["timeout", "-k", "10", "300", "rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", pmc_dir, "--"] + me + ["workload"]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    kt = {}
    for r in rows_of(trace_dir, "kernel_stats.csv"):
        if "planes_" in r["Name"] or "probe_read" in r["Name"]:
            kt[short(r["Name"])] = {k: r[k] for k in ("Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in r}
    res["kernel_trace"] = kt
    fetch = {}
    for r in rows_of(pmc_dir, "counter_collection.csv"):
        if r.get("Counter_Name") == "FETCH_SIZE" and ("planes_scan" in r["Kernel_Name"] or "probe_read" in r["Kernel_Name"]):
            fetch.setdefault(short(r["Kernel_Name"]), []).append(float(r["Counter_Value"]))
    # the workload runs rand4 (two planes, 256 MiB) first, then rand2 (one plane, 128 MiB): probe_read's launches split the same way
    res["fetch_size"] = {k: {"dispatches": len(v), "mean": sum(v) / len(v), "min": min(v), "max": max(v), "values": v} for k, v in fetch.items()}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
