#!/usr/bin/env python3
"""Edit distance for long patterns on packed texts, on the GPU: python tools/editl_probe.py [--out profiles/packed/packed_editl.json]

1 Gi symbols of rand4 and of rand2.  Numbers only, nothing is required of them:
  psearch_editl with m in MS and k in KS, the pattern cut from the text, with the cut-off (flags = 0) and with every block of
  every column (SMARTGPU_PEDITL_ALL_BLOCKS) — what the cut-off is worth —, and at m = 64, k <= 7 next to psearch_edit of the
  same pattern — what the block form costs on lengths both kernels can do; per call and per kernel.  Beside every cell the mean
  number of active blocks per column, counted on the CPU by tests/packed_editl_check.cpp on a random text of the same
  alphabet: per lane, and for 64 lanes that share one number as a wave of the kernel does.

The driver runs three steps, each a child process under its own `timeout`, and stops at the first that fails:
  1. the block counts (no GPU);
  2. `measure`   call times: the device's stream events around BATCH back-to-back calls, REPS repetitions after a warm-up, the
                 sides alternating inside every repetition;
  3. `rocprofv3 --kernel-trace --stats -- ... workload`   kernel times, a run of its own.
`render` writes the "Edit distance: long patterns" section of profiles/packed/RESULTS.md from the JSON file."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sets_probe import BATCH, commit, compare, make_text, rows_of, spread, timed  # noqa: E402

MS = (64, 65, 100, 150, 256)
KS = (0, 3, 7, 15, 31)
OLD_KS = (0, 3, 7)  # psearch_edit's, at m = 64
REPS, TRACE_REPS = 8, 8
TEXTS = (("rand4_1Gi", 4, 1 << 30), ("rand2_1Gi", 2, 1 << 30))
RUN = 512  # peditl.hpp kEditlRun: end positions a lane owns; it walks up to m + k symbols before them
SECTION = "## Edit distance: long patterns"


def sides_of(m):
    return [(side, k) for side in ("cut", "all") for k in KS] + ([("edit64", k) for k in OLD_KS] if m == 64 else [])


def call_of(side, P, pt, k):
    import smart_amd
    if side == "edit64":
        return lambda: smart_amd.psearch_edit(P, pt, k)[0]
    return lambda: smart_amd.psearch_editl(P, pt, k, all_blocks=side == "all")[0]


def measure(out):
    import smart_amd
    res = {"batch": BATCH, "reps": REPS, "unit": "ms per call (device events around %d back-to-back calls)" % BATCH, "run": RUN, "cells": []}
    for name, sigma, n in TEXTS:
        text, pt = make_text(sigma, n)
        for m in MS:
            P = text.read(n // 3 + 17, m)
            exact = smart_amd.psearch(P, pt)[0]
            sides = sides_of(m)
            t = {s: [] for s in sides}
            counts = {}
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                for side, k in (sides if rep % 2 else sides[::-1]):
                    ms, got = timed(call_of(side, P, pt, k))
                    assert got >= exact and (k or got == exact), (name, m, side, k, got, exact)
                    counts[(side, k)] = got
                    t[(side, k)].append(ms)
            for k in KS:
                assert counts[("cut", k)] == counts[("all", k)], (name, m, k, counts)
                c, a = spread(t[("cut", k)][1:]), spread(t[("all", k)][1:])
                cell = {"text": name, "n": n, "m": m, "k": k, "count": counts[("cut", k)], "cut_ms": c, "all_blocks_ms": a,
                        "warm_up_factor": (RUN + m + k) / RUN, "gsymbols_per_s_call": n / (c["median"] * 1e-3) / 1e9,
                        "all_over_cut": compare(c, a)}
                if ("edit64", k) in t:
                    assert counts[("edit64", k)] == counts[("cut", k)], (name, m, k, counts)
                    e = spread(t[("edit64", k)][1:])
                    cell["psearch_edit_ms"] = e
                    cell["cut_over_edit64"] = compare(e, c)
                res["cells"].append(cell)
                print("%-10s m=%-3d k=%-2d cut %.4f ms (%.1f Gsym/s, %d)  all blocks %.4f ms  x%.2f outside=%s%s" % (
                    name, m, k, c["median"], cell["gsymbols_per_s_call"], cell["count"], a["median"], cell["all_over_cut"]["ratio_of_medians"],
                    cell["all_over_cut"]["outside_spread"],
                    "  psearch_edit %.4f ms" % cell["psearch_edit_ms"]["median"] if "psearch_edit_ms" in cell else ""), flush=True)
        pt.free()
        text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per text, m and k, planes_editl_scan both ways (and planes_edit_scan at m = 64), TRACE_REPS + 1 times."""
    plan = []
    for name, sigma, n in TEXTS:
        text, pt = make_text(sigma, n)
        for m in MS:
            P = text.read(n // 3 + 17, m)
            for rep in range(TRACE_REPS + 1):
                for side, k in sides_of(m):
                    call_of(side, P, pt, k)()
                    plan.append([name, m, k, side, rep])
        pt.free()
        text.free()
    with open(plan_out, "w") as f:
        json.dump(plan, f)


def block_counts(scratch):
    """{(text, m, k): (per lane, per wave)} from tests/packed_editl_check.cpp, built without sanitizers."""
    exe = os.path.join(scratch, "packed_editl_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "packed_editl_check.cpp")])
    out = subprocess.check_output(["timeout", "-k", "10", "300", exe, "blocks"], text=True)
    got = {}
    for line in out.splitlines():
        w = line.split()
        if w and w[0] == "blocks":
            got[(w[1] + "_1Gi", int(w[2]), int(w[3]))] = (float(w[4]), float(w[5]))
    return got


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    print("== block counts", flush=True)
    blocks = block_counts(a.scratch)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "editl_trace"), os.path.join(a.scratch, "editl_plan.json")
    steps = [
        ("measure", ["timeout", "-k", "10", "420"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "editl_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if "planes_editl_scan" in r["Kernel_Name"] or "planes_edit_scan" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    for r, (name, m, k, side, rep) in zip(rows, launches):
        assert ("planes_edit_scan" in r["Kernel_Name"]) == (side == "edit64"), (r["Kernel_Name"], name, m, k, side, rep)
        if rep:
            per.setdefault((name, m, k, side), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for cell in res["cells"]:
        key = (cell["text"], cell["m"], cell["k"])
        c, al = spread(per[key + ("cut",)]), spread(per[key + ("all",)])
        cell["kernel_us"] = {"cut": c, "all_blocks": al, "all_over_cut": compare(c, al)}
        if key + ("edit64",) in per:
            e = spread(per[key + ("edit64",)])
            cell["kernel_us"]["planes_edit_scan"] = e
            cell["kernel_us"]["cut_over_edit64"] = compare(e, c)
        cell["gsymbols_per_s_kernel"] = cell["n"] / (c["median"] * 1e-6) / 1e9
        cell["active_blocks_per_lane"], cell["active_blocks_per_wave"] = blocks[key]
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/editl_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def render(a):
    """The "Edit distance: long patterns" section of RESULTS.md, appended (or replaced where it stands)."""
    res = json.load(open(a.out))
    fmt = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.0f [%.0f-%.0f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    rat = lambda c: "%.2f %s" % (c["ratio_of_medians"], "YES" if c["outside_spread"] else "no")  # noqa: E731
    note = lambda t: " (possibly flattered)" if t.startswith("rand2") else ""  # noqa: E731
    L = [SECTION, "",
         "`%s` -> `packed_editl.json`, taken on the kernels and library of commit %s.  1 Gi symbols; call: ms per call from the device's stream events around %d back-to-back calls, %d repetitions after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches per side after a warm-up.  median [min-max].  A ratio is followed by YES when the medians differ by more than the larger of the two spreads, by no otherwise.  The rand2 planes (128 MiB) are of Infinity-Cache size: possibly flattered." % (
             res.get("command"), res.get("commit"), res["batch"], res["reps"], res.get("trace_reps", 0)), "",
         "`psearch_editl` (`planes_editl_scan`) with the cut-off (flags = 0) and with every block of every column (`SMARTGPU_PEDITL_ALL_BLOCKS`), the pattern cut from the text.  A lane owns a run of %d end positions and walks up to m + k symbols before it: the warm-up factor is (%d + m + k) / %d.  blocks: the mean number of active blocks per column, counted on the CPU (`tests/packed_editl_check.cpp blocks`) on a random text of the same alphabet and a random pattern, per lane / for 64 lanes that share one number, as a wave of the kernel does; W: the blocks of the pattern, what all blocks computes.  Recorded as measured; nothing is required of it." % (res["run"], res["run"], res["run"]), "",
         "| text | m | k | warm-up | occurrences | W | blocks (lane / wave) | cut-off, ms | all blocks, ms | all / cut | Gsym/s (call) | cut-off kernel, us | all blocks kernel, us | all / cut | Gsym/s (kernel) |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        k = c.get("kernel_us")
        L.append("| %s%s | %d | %d | %.2f | %d | %d | %s | %s | %s | %s | %.1f | %s | %s | %s | %s |" % (
            c["text"], note(c["text"]), c["m"], c["k"], c["warm_up_factor"], c["count"], (c["m"] + 31) // 32,
            "%.2f / %.2f" % (c["active_blocks_per_lane"], c["active_blocks_per_wave"]) if "active_blocks_per_lane" in c else "not counted",
            fmt(c["cut_ms"]), fmt(c["all_blocks_ms"]), rat(c["all_over_cut"]), c["gsymbols_per_s_call"],
            fus(k["cut"]) if k else "not measured", fus(k["all_blocks"]) if k else "not measured", rat(k["all_over_cut"]) if k else "",
            "%.1f" % c["gsymbols_per_s_kernel"] if k else ""))
    L += ["", "The block form against the kernel that keeps the whole column in two dwords, on the length both can do (m = 64, the same pattern; `psearch_edit`, `planes_edit_scan`):", "",
          "| text | k | psearch_edit, ms | psearch_editl, ms | editl / edit | planes_edit_scan, us | planes_editl_scan, us | editl / edit |", "|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        if "psearch_edit_ms" in c:
            k = c.get("kernel_us")
            L.append("| %s%s | %d | %s | %s | %s | %s | %s | %s |" % (
                c["text"], note(c["text"]), c["k"], fmt(c["psearch_edit_ms"]), fmt(c["cut_ms"]), rat(c["cut_over_edit64"]),
                fus(k["planes_edit_scan"]) if k else "not measured", fus(k["cut"]) if k else "not measured", rat(k["cut_over_edit64"]) if k else ""))
    L += ["", "Choices that are NOT measured: the run of %d end positions per lane against other lengths, pieces of 128 symbols loaded as they are reached (no prefetch of the next piece), the occupancy (`__launch_bounds__(256, 8)`, 8 workgroups per CU), the number of active blocks per wave ON the device (the figures above are the CPU's), the find form's speed and the share of the host's sort in it, texts beyond 1 Gi symbols." % res["run"]]
    path = os.path.join(os.path.dirname(a.out), "RESULTS.md")
    if not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", "packed", "RESULTS.md")
    text = open(path).read()
    at = text.find("\n" + SECTION)
    if at >= 0:
        end = text.find("\n## ", at + 1)
        text = text[:at] + (text[end:] if end >= 0 else "\n")
    text = text.rstrip("\n") + "\n\n" + "\n".join(L) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("rendered the section '%s' of %s" % (SECTION, path))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_editl.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "editl_probe"))
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
