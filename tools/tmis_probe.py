#!/usr/bin/env python3
"""Mismatches on byte texts, on the GPU: python tools/tmis_probe.py [--out profiles/tedit/tmis.json]

1 GiB texts, m in MS, k in KS, the pattern cut from the text.  Numbers only, nothing is required of them:
  1. scan      search_mis against search_edit (text_edit_scan, the same tile, P and k) on rand4, rand128 and the English
               corpus tiled to 1 GiB;
  2. packed    psearch_mis on the packed text of the same rand4 bytes, the same P and k: the planes decide 32 positions
               per instruction — the ratio says when to pack;
  3. find      find_mis against search_mis at 2^20 occurrences: a unit of 1 KiB over 128 values with one copy of the
               pattern (k // 2 substitutions) tiled to 1 GiB.
Per call: the host clock around one synchronous call, REPS calls after a warm-up, the sides alternating.  Per kernel: a
`rocprofv3 --kernel-trace` run of its own, TRACE_REPS dispatches after a warm-up.  Medians with [min-max].

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails.  `render` writes
the section "Mismatches" of profiles/tedit/RESULTS.md from the JSON file."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sets_probe import commit, compare, rows_of, spread  # noqa: E402

MS = (8, 20, 32, 33, 64)
KS = (0, 1, 3, 7)
N = 1 << 30
REPS, TRACE_REPS = 7, 5
TEXTS = ("rand4", "rand128", "english")
FIND_CASES = ((20, 2), (64, 7))
FIND_UNIT = 1024
SECTION = "## Mismatches"
KERNEL_OF = {"search_mis": "text_mis_scan", "search_edit": "text_edit_scan", "psearch_mis": "planes_mis_scan"}


def make_text(name):
    import smart_amd
    from smart_amd import corpus
    if name.startswith("rand"):
        sigma = int(name[4:])
        return smart_amd.Text.generate(0x5EED0400 + sigma, sigma, N)
    return smart_amd.Text.upload_tiled(corpus.english_unit(), N)


def sides(name, text):
    """[(side, call(P, k) -> count)] for a text: search_mis, search_edit, and on rand4 psearch_mis on the same bytes packed."""
    import smart_amd
    out = [("search_mis", lambda P, k: smart_amd.search_mis(P, text, k)), ("search_edit", lambda P, k: smart_amd.search_edit(P, text, k))]
    pt = None
    if name == "rand4":
        pt = smart_amd.PackedText.pack(text)
        out.append(("psearch_mis", lambda P, k: smart_amd.psearch_mis(P, pt, k)[0]))
    return out, pt


def find_text(m, k):
    """(text, P): 2^20 copies of a 1 KiB unit over 128 values that holds P once, with k // 2 substitutions."""
    import numpy as np
    import smart_amd
    rng = np.random.default_rng(7000 + m)
    unit = rng.integers(0, 128, FIND_UNIT).astype(np.uint8)
    P = rng.integers(0, 128, m).astype(np.uint8)
    W = P.copy()
    W[1:1 + k // 2] ^= 0x80  # values the unit does not hold
    unit[100:100 + m] = W
    return smart_amd.Text.upload_tiled(unit, N), P


def clocked(fn):
    t0 = time.perf_counter()
    got = fn()
    return (time.perf_counter() - t0) * 1e3, got


def measure(out):
    import smart_amd
    res = {"reps": REPS, "unit": "ms per call (host clock around one synchronous call)", "n": N, "cells": [], "find": []}
    for name in TEXTS:
        text = make_text(name)
        calls, pt = sides(name, text)
        for m in MS:
            P = text.read(N // 3 + 17, m)
            for k in KS:
                t, counts = {s: [] for s, _ in calls}, {}
                for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                    for s, call in (calls if rep % 2 else calls[::-1]):
                        ms, counts[s] = clocked(lambda: call(P, k))
                        t[s].append(ms)
                assert counts["search_mis"] >= 1 and counts["search_edit"] >= counts["search_mis"], (name, m, k, counts)
                assert counts.get("psearch_mis", counts["search_mis"]) == counts["search_mis"], (name, m, k, counts)  # both Hamming kernels count the same starts
                cell = {"text": name, "m": m, "k": k, "count": counts["search_mis"], "edit_count": counts["search_edit"],
                        "call_ms": {s: spread(v[1:]) for s, v in t.items()}}
                cell["gb_per_s_call"] = N / (cell["call_ms"]["search_mis"]["median"] * 1e-3) / 1e9
                res["cells"].append(cell)
                print("%-8s m=%-2d k=%d %s  %.0f GB/s, %d starts" % (name, m, k, "  ".join("%s %.3f ms" % (s, v["median"]) for s, v in cell["call_ms"].items()),
                                                                    cell["gb_per_s_call"], cell["count"]), flush=True)
        if pt:
            pt.free()
        text.free()
    for m, k in FIND_CASES:
        text, P = find_text(m, k)
        t = {"search_mis": [], "find_mis": []}
        for rep in range(REPS + 1):
            ms, count = clocked(lambda: smart_amd.search_mis(P, text, k))
            t["search_mis"].append(ms)
            ms, (pos, dist) = clocked(lambda: smart_amd.find_mis(P, text, k, cap=1 << 21))
            t["find_mis"].append(ms)
            assert count == len(pos) == N // FIND_UNIT and int(pos[0]) == 100 and int(dist[0]) == k // 2, (m, k, count, len(pos))
        cell = {"m": m, "k": k, "count": count, "call_ms": {s: spread(v[1:]) for s, v in t.items()}}
        cell.update(compare(cell["call_ms"]["search_mis"], cell["call_ms"]["find_mis"]))
        res["find"].append(cell)
        print("find m=%-2d k=%d search_mis %.3f ms  find_mis %.3f ms  x%.2f, %d starts" % (
            m, k, cell["call_ms"]["search_mis"]["median"], cell["call_ms"]["find_mis"]["median"], cell["ratio_of_medians"], count), flush=True)
        text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per text, m and k, every side's count kernel TRACE_REPS + 1 times."""
    plan = []
    for name in TEXTS:
        text = make_text(name)
        calls, pt = sides(name, text)
        for m in MS:
            P = text.read(N // 3 + 17, m)
            for k in KS:
                for rep in range(TRACE_REPS + 1):
                    for s, call in calls:
                        call(P, k)
                        plan.append([name, m, k, s, rep])
        if pt:
            pt.free()
        text.free()
    with open(plan_out, "w") as f:
        json.dump(plan, f)


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "tmis_trace"), os.path.join(a.scratch, "tmis_plan.json")
    steps = [
        ("measure", ["timeout", "-k", "10", "300"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "tmis_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if any(kn in r["Kernel_Name"] for kn in KERNEL_OF.values())]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    raw = os.path.join(os.path.dirname(a.out), "raw")
    os.makedirs(raw, exist_ok=True)
    with open(os.path.join(raw, "tmis_scan_kernels.csv"), "w") as f:
        f.write("text,m,k,side,rep,kernel,us\n")
        for r, (name, m, k, side, rep) in zip(rows, launches):
            assert KERNEL_OF[side] in r["Kernel_Name"], (r["Kernel_Name"], name, m, k, side, rep)
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            f.write("%s,%d,%d,%s,%d,%s,%.3f\n" % (name, m, k, side, rep, KERNEL_OF[side], us))
            if rep:
                per.setdefault((name, m, k, side), []).append(us)
    for cell in res["cells"]:
        cell["kernel_us"] = {s: spread(per[(cell["text"], cell["m"], cell["k"], s)]) for s in cell["call_ms"]}
        cell["gb_per_s_kernel"] = N / (cell["kernel_us"]["search_mis"]["median"] * 1e-6) / 1e9
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/tmis_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def render(a):
    res = json.load(open(a.out))
    fms = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.0f [%.0f-%.0f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    traced = all("kernel_us" in c for c in res["cells"])
    L = [SECTION, "",
         "`%s` -> `%s` (the traced dispatches one by one: `raw/tmis_scan_kernels.csv`), taken on the kernels and library of commit %s.  1 GiB texts.  call: ms per call, the host clock around one synchronous call, %d calls after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches after a warm-up.  median [min-max]: the bracket is the run-to-run spread.  outside: the medians differ by more than the larger of the two spreads.  Recorded as measured; nothing is required of these numbers." % (
             res.get("command", "python tools/tmis_probe.py"), os.path.basename(a.out), res.get("commit", "?"), res["reps"], res.get("trace_reps", 0)), "",
         "### text_mis_scan against text_edit_scan: the same tile, the same P and k", "",
         "| text | m | k | starts | search_mis, ms per call | search_edit, ms per call | mis / edit | outside | text_mis_scan, us | text_edit_scan, us | mis / edit | outside | GB/s (kernel) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        call = compare(c["call_ms"]["search_edit"], c["call_ms"]["search_mis"])
        kern = compare(c["kernel_us"]["search_edit"], c["kernel_us"]["search_mis"]) if traced else None
        L.append("| %s | %d | %d | %d | %s | %s | %.2f | %s | %s | %s | %s | %s | %s |" % (
            c["text"], c["m"], c["k"], c["count"], fms(c["call_ms"]["search_mis"]), fms(c["call_ms"]["search_edit"]), call["ratio_of_medians"], "YES" if call["outside_spread"] else "no",
            fus(c["kernel_us"]["search_mis"]) if traced else "not measured", fus(c["kernel_us"]["search_edit"]) if traced else "not measured",
            "%.2f" % kern["ratio_of_medians"] if kern else "", ("YES" if kern["outside_spread"] else "no") if kern else "", "%.0f" % c["gb_per_s_kernel"] if traced else ""))
    L += ["", "### Against psearch_mis on the same rand4 bytes, packed", "",
          "The planes decide 32 start positions per instruction (`planes_mis_scan`); a lane of `text_mis_scan` walks its text a byte at a time.  bytes / packed says what packing a text of at most four values buys.", "",
          "| m | k | psearch_mis, ms per call | search_mis, ms per call | bytes / packed | outside | planes_mis_scan, us | text_mis_scan, us | bytes / packed | outside |", "|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        if c["text"] == "rand4":
            call = compare(c["call_ms"]["psearch_mis"], c["call_ms"]["search_mis"])
            kern = compare(c["kernel_us"]["psearch_mis"], c["kernel_us"]["search_mis"]) if traced else None
            L.append("| %d | %d | %s | %s | %.2f | %s | %s | %s | %s | %s |" % (
                c["m"], c["k"], fms(c["call_ms"]["psearch_mis"]), fms(c["call_ms"]["search_mis"]), call["ratio_of_medians"], "YES" if call["outside_spread"] else "no",
                fus(c["kernel_us"]["psearch_mis"]) if traced else "not measured", fus(c["kernel_us"]["search_mis"]) if traced else "not measured",
                "%.2f" % kern["ratio_of_medians"] if kern else "", ("YES" if kern["outside_spread"] else "no") if kern else ""))
    L += ["", "### find_mis against search_mis at 2^20 occurrences", "",
          "A 1 KiB unit over 128 values with one copy of the pattern, tiled to 1 GiB; per call by the host clock, the list's copy to the host, the ordering of the spans and the unpacking included.", "",
          "| m | k | starts | search_mis, ms per call | find_mis, ms per call | find / search | outside |", "|---|---|---|---|---|---|---|"]
    for c in res["find"]:
        L.append("| %d | %d | %d | %s | %s | %.2f | %s |" % (c["m"], c["k"], c["count"], fms(c["call_ms"]["search_mis"]), fms(c["call_ms"]["find_mis"]), c["ratio_of_medians"], "YES" if c["outside_spread"] else "no"))
    L += ["", "### NOT measured", "",
          "Four workgroups per CU and `__launch_bounds__(256, 4)` against other occupancies; the run of 128 end positions per lane; the walk from a workgroup-wide start in one rolled dword loop against an unrolled walk with per-lane edges; the compressed code object's load time (once per process); the classes calls (the kernels are the same, the host builds another table); `text_mis_find`'s kernel time (no trace of it) and the host ordering's share in the find; texts beyond 1 GiB (the at-size test checks answers beyond 2^32, not times); hardware counters.", ""]
    path = os.path.join(ROOT, "profiles", "tedit", "RESULTS.md")
    text = open(path).read()
    at = text.find("\n" + SECTION)
    if at >= 0:
        end = text.find("\n## ", at + 1)
        text = text[:at] + (text[end:] if end >= 0 else "\n")
    text = text.rstrip("\n") + "\n\n" + "\n".join(L) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("rendered " + path)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tedit", "tmis.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "tmis_probe"))
    ap.add_argument("--commit", help="the commit the numbers are taken on (default: git rev-parse HEAD)")
    a = ap.parse_args()
    a.out, a.scratch = os.path.abspath(a.out), os.path.abspath(a.scratch)
    if a.step == "measure":
        return measure(a.out)
    if a.step == "workload":
        return workload(a.out)
    if a.step == "render":
        return render(a)
    return driver(a) or render(a)


if __name__ == "__main__":
    sys.exit(main())
