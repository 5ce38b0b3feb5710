#!/usr/bin/env python3
"""Packed texts (bit planes) against the byte text, on the GPU: python tools/packed_probe.py [--out profiles/packed/packed_text.json]

`python tools/packed_probe.py find` is the same for POSITIONS (pfind against find on the byte text, planes_find against
planes_scan, FETCH_SIZE of planes_find): profiles/packed/packed_find.json and the "Positions" section of RESULTS.md.
`python tools/packed_probe.py find-asm --asm-old OLD.s --asm-new NEW.s` (no GPU) adds tools/asm_stats.py --diff of the
parent's k_planes assembly against this tree's to that file and renders the section again.

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


FIND_MS = (4, 8, 16, 32, 256, 4096)


def find_pattern(text, n, m):
    return text.read(n // 3 + 17, m)


def find_measure(out):
    """Whole calls: smartgpu_pfind64 on the planes against smartgpu_find64 on the byte text of the same symbols, wall clock
    around the call (it ends in a synchronisation and includes the copy and the ordering), the two alternating, REPS
    repetitions after a warm-up, buffers allocated before."""
    import ctypes as C
    import numpy as np
    import smart_amd
    L = smart_amd.lib()
    res = {"reps": REPS, "unit": "ms per call, wall clock", "cells": []}
    for name, sigma, n in TEXTS:
        text = smart_amd.Text.generate(0x5EED0400 + sigma, sigma, n)
        pt = smart_amd.PackedText.pack(text)
        for m in FIND_MS:
            P = find_pattern(text, n, m)
            count = smart_amd.psearch(P, pt)[0]
            cell = {"text": name, "m": m, "count": count, "bytes_copied": 8 * count,
                    "sparse": bool(sigma ** m > 16384)}  # expected occurrences per wave and trip (2 x 8192 start positions) below one
            a, b = np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.uint64)
            c = C.c_uint64(0)
            packed, byte = [], []
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped (and compared)
                t0 = time.perf_counter()
                rc = L.smartgpu_pfind64(P.ctypes.data, m, pt._h, 0, n, a.ctypes.data, count + 1, C.byref(c))
                t1 = time.perf_counter()
                assert rc == 0 and c.value == count, (name, m, rc, c.value, count)
                t2 = time.perf_counter()
                rc = L.smartgpu_find64(P.ctypes.data, m, text._h, 0, n, b.ctypes.data, count + 1, C.byref(c))
                t3 = time.perf_counter()
                assert rc == 0 and c.value == count, (name, m, rc, c.value, count)
                if rep == 0:
                    assert np.array_equal(a, b), (name, m)
                else:
                    packed.append((t1 - t0) * 1e3)
                    byte.append((t3 - t2) * 1e3)
            p, q = spread(packed), spread(byte)
            cell.update({"pfind_ms": p, "find_ms": q, "ratio_of_medians": q["median"] / p["median"],
                         "faster": bool(q["median"] - p["median"] > max(p["max"] - p["min"], q["max"] - q["min"]))})
            res["cells"].append(cell)
            print("%-10s m=%-5d count %-9d pfind %.3f [%.3f-%.3f] ms  find %.3f [%.3f-%.3f] ms  x%.2f  faster=%s" % (
                name, m, count, p["median"], p["min"], p["max"], q["median"], q["min"], q["max"], cell["ratio_of_medians"], cell["faster"]), flush=True)
        pt.free()
        text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def find_workload(which, plan_out=None):
    """What the profiler runs look at.  `trace`: every text, every m — planes_scan (psearch) and planes_find (pfind with
    room for every position) alternating, REPS + 1 times; the order of the launches goes to plan_out, the kernel trace is
    matched against it.  `pmc`: 1 Gi of rand4 and of rand2 — a plain read of the planes, then planes_find."""
    import smart_amd
    plan = []
    for name, sigma, n in (TEXTS if which == "trace" else TEXTS[:2]):
        text = smart_amd.Text.generate(0x5EED0400 + sigma, sigma, n)
        with smart_amd.PackedText.pack(text) as pt:
            if which == "pmc":
                pt.probe_read_gbs(4)
            for m in (FIND_MS if which == "trace" else (8, 32, 256)):
                P = find_pattern(text, n, m)
                count = smart_amd.psearch(P, pt)[0]
                plan.append([name, m, "scan", 0])
                for rep in range(REPS + 1 if which == "trace" else 4):
                    smart_amd.psearch(P, pt)
                    plan.append([name, m, "scan", rep])
                    got, c = smart_amd.pfind(P, pt, cap=count + 1)
                    assert c == count and got is not None
                    plan.append([name, m, "find", rep])
        text.free()
    if plan_out:
        with open(plan_out, "w") as f:
            json.dump(plan, f)


def find_driver(a):
    """The `find` step: three children, each under its own timeout, stopping at the first failure; one JSON file out and the
    "Positions" section of RESULTS.md rendered from it."""
    out = os.path.join(os.path.dirname(a.out), "packed_find.json")
    os.makedirs(a.scratch, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, pmc_dir, plan = os.path.join(a.scratch, "find_trace"), os.path.join(a.scratch, "find_pmc"), os.path.join(a.scratch, "find_plan.json")
    steps = [
        ("find measure", ["timeout", "-k", "10", "420"] + me + ["find-measure", "--out", out]),
        ("find kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["find-workload-trace", "--out", plan]),
        ("find FETCH_SIZE", ["timeout", "-k", "10", "240", "rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", pmc_dir, "--"] + me + ["find-workload-pmc"]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "find measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(out))
    # kernel times: the trace's planes_scan / planes_find dispatches in start order against the order the workload launched them
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if "planes_scan" in r["Kernel_Name"] or "planes_find" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    for r, (name, m, kind, rep) in zip(rows, launches):
        assert ("planes_find" in r["Kernel_Name"]) == (kind == "find"), (r["Kernel_Name"], name, m, kind, rep)
        if rep:
            per.setdefault((name, m), {"scan": [], "find": []})[kind].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for cell in res["cells"]:
        k = per.get((cell["text"], cell["m"]))
        if not k:
            continue
        s, f = spread(k["scan"]), spread(k["find"])
        cell["kernel_us"] = {"planes_scan": s, "planes_find": f, "find_over_scan": f["median"] / s["median"],
                             "within_spread": bool(f["median"] - s["median"] <= max(s["max"] - s["min"], f["max"] - f["min"]))}
    fetch = {}
    for r in rows_of(pmc_dir, "counter_collection.csv"):
        if r.get("Counter_Name") == "FETCH_SIZE" and any(k in r["Kernel_Name"] for k in ("planes_find", "planes_scan", "probe_read")):
            fetch.setdefault(short(r["Kernel_Name"]), []).append(float(r["Counter_Value"]))
    res["fetch_size"] = {k: {"dispatches": len(v), "mean": sum(v) / len(v), "min": min(v), "max": max(v), "values": v} for k, v in fetch.items()}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + out)
    return 0


def find_render(a):
    """The "Positions" section of RESULTS.md (the file's last), from packed_find.json."""
    d = os.path.dirname(a.out)
    res = json.load(open(os.path.join(d, "packed_find.json")))
    fmt = lambda v, u=1.0: "%.3f [%.3f-%.3f]" % (v["median"] / u, v["min"] / u, v["max"] / u)  # noqa: E731
    L = ["## Positions", "",
         "`python tools/packed_probe.py find` -> `packed_find.json`; %d repetitions after a warm-up, the two paths alternating inside one process, median [min-max]." % res["reps"],
         "Whole call: `smartgpu_pfind64` on the planes against `smartgpu_find64` on the byte text of the same symbols, wall clock around the call (synchronisation, copy and ordering included), room for every position.  Kernel: `planes_find` against `planes_scan`, same pattern, same text, from a `rocprofv3 --kernel-trace` run of its own.  sparse: fewer than one expected occurrence per wave and trip.  faster: `find` - `pfind` exceeds the larger of the two spreads; within: `planes_find` - `planes_scan` does not.", "",
         "| text | m | occurrences | sparse | pfind, ms | find (byte text), ms | find / pfind | faster | planes_scan, us | planes_find, us | find / scan | within the spread |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        k = c.get("kernel_us")
        L.append("| %s | %d | %d | %s | %s | %s | %.2f | %s | %s | %s | %s | %s |" % (
            c["text"], c["m"], c["count"], "yes" if c["sparse"] else "no", fmt(c["pfind_ms"]), fmt(c["find_ms"]), c["ratio_of_medians"], "yes" if c["faster"] else "no",
            fmt(k["planes_scan"]) if k else "not measured", fmt(k["planes_find"]) if k else "not measured", "%.3f" % k["find_over_scan"] if k else "", ("yes" if k["within_spread"] else "NO") if k else ""))
    done = res["cells"]
    req = [c for c in done if c["text"] == "rand4_8Gi" and c["sparse"]]
    L += ["", "Required — `pfind` faster than `find` on the sparse cells of the 8 Gi text (2 GiB of planes, far beyond the Infinity Cache): %s." % (
        "holds in all %d cells (%.1f-%.1f x)" % (len(req), min(c["ratio_of_medians"] for c in req), max(c["ratio_of_medians"] for c in req)) if req and all(c["faster"] for c in req)
        else "MISSED in m = " + ", ".join(str(c["m"]) for c in req if not c["faster"]))]
    miss = [c for c in done if c["sparse"] and c.get("kernel_us") and not c["kernel_us"]["within_spread"]]
    L.append("Sparse cells where `planes_find` is slower than `planes_scan` by more than the larger spread: %s." % (
        ", ".join("%s m = %d (%.3f x)" % (c["text"], c["m"], c["kernel_us"]["find_over_scan"]) for c in miss) if miss else "none"))
    if miss:
        L.append("The cause is the cursor, not the registers (35 / 49 VGPRs against 32 / 45, the same 8 workgroups per CU; the cells with one occurrence are within the spread): in these cells nearly every occurrence is a span of its own, and every span with an occurrence costs one returning atomic on the ONE cursor — (`planes_find` - `planes_scan`) / occurrences = %s.  The dense cells show the same rate per span.  It stays as a finding: one atomic per wave and chunk row is the form this kernel was asked to have; fewer, larger reservations (per workgroup, or per wave and trip) are not built." % (
            ", ".join("%.1f ns" % (1e3 * (c["kernel_us"]["planes_find"]["median"] - c["kernel_us"]["planes_scan"]["median"]) / c["count"]) for c in miss)))
    L.append("The 1 Gi rows carry the Infinity-Cache caveat of the counting table.  Dense cells are bound by output and ordering; nothing is required of them.")
    dense = max(done, key=lambda c: c["count"])
    k = dense.get("kernel_us")
    L += ["", "What ordering costs, on the densest cell measured (%s, m = %d, %d occurrences): the call takes %s ms by wall clock, the kernel %s, %d bytes are copied to the host; the rest is the copy to the host (through one 32 MiB pinned buffer, part by part, copy and memcpy not overlapped) and the pass that finds and orders the spans." % (
        dense["text"], dense["m"], dense["count"], fmt(dense["pfind_ms"]), (fmt(k["planes_find"], 1e3) + " ms") if k else "was not measured", dense["bytes_copied"])]
    fs = res.get("fetch_size", {})
    if fs:
        L += ["", "HBM traffic, `rocprofv3 --pmc FETCH_SIZE`, counters only, a run of its own (1 Gi of rand4, then of rand2; `probe_read` is a plain read of the same planes, its first half of dispatches on two planes, the second on one): " +
              "; ".join("`%s` mean %.0f (min %.0f, max %.0f, %d dispatches)" % (n, v["mean"], v["min"], v["max"], v["dispatches"]) for n, v in sorted(fs.items())) + "."]
        pr = next((v["values"] for n, v in fs.items() if "probe_read" in n), None)
        if pr and len(pr) % 2 == 0:
            h = len(pr) // 2
            for n, v in sorted(fs.items()):
                if "planes_find<2>" in n:
                    L.append("`planes_find<2>` / `probe_read` on two planes: %.3f." % (v["mean"] / (sum(pr[:h]) / h)))
                if "planes_find<1>" in n:
                    L.append("`planes_find<1>` / `probe_read` on one plane: %.3f." % (v["mean"] / (sum(pr[h:]) / h)))
    if res.get("asm_diff"):
        L += ["", "`python tools/asm_stats.py --diff` of the parent's `k_planes` assembly against this one (gfx950, cross-compiled):", "", "```"] + res["asm_diff"] + ["```"]
    path = os.path.join(d, "RESULTS.md")
    if not os.path.exists(path):  # --out elsewhere: the section still belongs to the committed file
        path = os.path.join(ROOT, "profiles", "packed", "RESULTS.md")
    text = open(path).read()
    at = text.find("\n## Positions")
    text = (text[:at] if at >= 0 else text.rstrip("\n") + "\n") + "\n" + "\n".join(L) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("rendered the Positions section of " + path)
    return 0


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
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "find", "find-measure", "find-workload-trace", "find-workload-pmc", "find-render", "find-asm"))
    ap.add_argument("--asm-old", help="find-asm: the parent commit's k_planes-hip-amdgcn-amd-amdhsa-gfx950.s (make -C smart_amd/csrc asm)")
    ap.add_argument("--asm-new", help="find-asm: the same file of this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_text.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "packed_probe"))
    a = ap.parse_args()
    a.out, a.scratch = os.path.abspath(a.out), os.path.abspath(a.scratch)
    if a.step == "measure":
        return measure(a.out)
    if a.step == "workload":
        return workload()
    if a.step == "find-measure":
        return find_measure(a.out)
    if a.step == "find-workload-trace":
        return find_workload("trace", a.out)
    if a.step == "find-workload-pmc":
        return find_workload("pmc")
    if a.step == "find":
        rc = find_driver(a)
        return rc or find_render(a)
    if a.step == "find-render":
        return find_render(a)
    if a.step == "find-asm":  # no GPU: tools/asm_stats.py --diff of two cross-compiled assemblies into packed_find.json, section rendered again
        out = os.path.join(os.path.dirname(a.out), "packed_find.json")
        lines = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "asm_stats.py"), "--diff", a.asm_old, a.asm_new], text=True).splitlines()
        res = json.load(open(out))
        res["asm_diff"] = [ln.rstrip() for ln in lines]
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        return find_render(a)
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
