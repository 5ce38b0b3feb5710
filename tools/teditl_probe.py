#!/usr/bin/env python3
"""Edit distance for long patterns on byte texts, on the GPU: python tools/teditl_probe.py [--out profiles/tedit/teditl.json]

1 GiB of rand128, of the English corpus tiled, and of rand4; m in MS, k in KS, the pattern cut from the text.  Numbers only,
nothing is required of them:
  cut / all   search_editl with the cut-off (flags = 0) and with every block of every column (SMARTGPU_EDITL_ALL_BLOCKS): what
              the cut-off is worth, in every cell;
  edit64      at m = 64, k <= 7: search_edit of the same pattern (text_edit_scan, the kernel that keeps the whole column in
              two dwords and owns runs of 128): what the block form costs on lengths both kernels can do;
  packed      on rand4: psearch_editl on the same bytes packed, same P and k (planes_editl_scan): the same recurrence and the
              same run of 512, the text from two bit planes and the masks from kernel arguments — the price of bytes.
Per call: the host clock around one synchronous call, REPS calls after a warm-up, the sides alternating.  Per kernel: a
`rocprofv3 --kernel-trace` run of its own, TRACE_REPS dispatches after a warm-up.  Medians with [min-max].

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails.  `render` writes
the "Long patterns" section of profiles/tedit/RESULTS.md from the JSON file."""
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

MS = (64, 65, 100, 150, 256)
KS = (0, 3, 7, 15, 31)
OLD_KS = (0, 3, 7)  # search_edit's, at m = 64
N = 1 << 30
REPS, TRACE_REPS = 7, 5
RUN = 512  # teditl_host.hpp kTEditlRun: end positions a lane owns; it walks up to m + k bytes before them
TEXTS = ("rand128", "english", "rand4")
SECTION = "## Long patterns"
KERNEL_OF = {"cut": "text_editl_scan", "all": "text_editl_scan", "edit64": "text_edit_scan", "packed": "planes_editl_scan"}


def make_text(name):
    import smart_amd
    from smart_amd import corpus
    if name.startswith("rand"):
        sigma = int(name[4:])
        return smart_amd.Text.generate(0x5EED0400 + sigma, sigma, N)
    return smart_amd.Text.upload_tiled(corpus.english_unit(), N)


def sides_of(name, m):
    s = [(side, k) for side in ("cut", "all") for k in KS]
    if m == 64:
        s += [("edit64", k) for k in OLD_KS]
    if name == "rand4":
        s += [("packed", k) for k in KS]
    return s


def call_of(side, P, text, pt, k):
    import smart_amd
    if side == "edit64":
        return lambda: smart_amd.search_edit(P, text, k)
    if side == "packed":
        return lambda: smart_amd.psearch_editl(P, pt, k)[0]
    return lambda: smart_amd.search_editl(P, text, k, all_blocks=side == "all")


def clocked(fn):
    t0 = time.perf_counter()
    got = fn()
    return (time.perf_counter() - t0) * 1e3, got


def measure(out):
    import smart_amd
    res = {"reps": REPS, "unit": "ms per call (host clock around one synchronous call)", "run": RUN, "n": N, "cells": []}
    for name in TEXTS:
        text = make_text(name)
        pt = smart_amd.PackedText.pack(text) if name == "rand4" else None
        for m in MS:
            P = text.read(N // 3 + 17, m)
            sides = sides_of(name, m)
            t, counts = {s: [] for s in sides}, {}
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                for side, k in (sides if rep % 2 else sides[::-1]):
                    ms, counts[(side, k)] = clocked(call_of(side, P, text, pt, k))
                    t[(side, k)].append(ms)
            for k in KS:
                same = [counts[(s, kk)] for s, kk in sides if kk == k]
                assert len(set(same)) == 1 and same[0] >= 1, (name, m, k, counts)  # every kernel counts the same ends
                c, al = spread(t[("cut", k)][1:]), spread(t[("all", k)][1:])
                cell = {"text": name, "m": m, "k": k, "count": counts[("cut", k)], "warm_up_factor": (RUN + m + k) / RUN,
                        "call_ms": {"cut": c, "all": al}, "all_over_cut": compare(c, al), "gb_per_s_call": N / (c["median"] * 1e-3) / 1e9}
                for side in ("edit64", "packed"):
                    if (side, k) in t:
                        cell["call_ms"][side] = spread(t[(side, k)][1:])
                        cell["cut_over_" + side] = compare(cell["call_ms"][side], c)
                res["cells"].append(cell)
                print("%-8s m=%-3d k=%-2d cut %.3f ms (%.0f GB/s, %d ends)  all blocks %.3f ms  x%.2f outside=%s%s" % (
                    name, m, k, c["median"], cell["gb_per_s_call"], cell["count"], al["median"], cell["all_over_cut"]["ratio_of_medians"],
                    cell["all_over_cut"]["outside_spread"],
                    "".join("  %s %.3f ms" % (s, cell["call_ms"][s]["median"]) for s in ("edit64", "packed") if s in cell["call_ms"])), flush=True)
        if pt:
            pt.free()
        text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per text, m and k, every side's count kernel TRACE_REPS + 1 times."""
    import smart_amd
    plan = []
    for name in TEXTS:
        text = make_text(name)
        pt = smart_amd.PackedText.pack(text) if name == "rand4" else None
        for m in MS:
            P = text.read(N // 3 + 17, m)
            for rep in range(TRACE_REPS + 1):
                for side, k in sides_of(name, m):
                    call_of(side, P, text, pt, k)()
                    plan.append([name, m, k, side, rep])
        if pt:
            pt.free()
        text.free()
    with open(plan_out, "w") as f:
        json.dump(plan, f)


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "teditl_trace"), os.path.join(a.scratch, "teditl_plan.json")
    steps = [
        ("measure", ["timeout", "-k", "10", "300"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "teditl_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    names = set(KERNEL_OF.values())
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if any(kn + "<" in r["Kernel_Name"] or kn + "I" in r["Kernel_Name"] for kn in names)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    raw = os.path.join(os.path.dirname(a.out), "raw")
    os.makedirs(raw, exist_ok=True)
    with open(os.path.join(raw, "teditl_scan_kernels.csv"), "w") as f:
        f.write("text,m,k,side,rep,kernel,us\n")
        for r, (name, m, k, side, rep) in zip(rows, launches):
            assert KERNEL_OF[side] in r["Kernel_Name"], (r["Kernel_Name"], name, m, k, side, rep)
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            f.write("%s,%d,%d,%s,%d,%s,%.3f\n" % (name, m, k, side, rep, KERNEL_OF[side], us))
            if rep:
                per.setdefault((name, m, k, side), []).append(us)
    for cell in res["cells"]:
        key = (cell["text"], cell["m"], cell["k"])
        ku = {s: spread(per[key + (s,)]) for s in cell["call_ms"]}
        cell["kernel_us"] = ku
        cell["kernel_all_over_cut"] = compare(ku["cut"], ku["all"])
        for side in ("edit64", "packed"):
            if side in ku:
                cell["kernel_cut_over_" + side] = compare(ku[side], ku["cut"])
        cell["gb_per_s_kernel"] = N / (ku["cut"]["median"] * 1e-6) / 1e9
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/teditl_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def render(a):
    """The "Long patterns" section of profiles/tedit/RESULTS.md, appended (or replaced where it stands)."""
    res = json.load(open(a.out))
    fms = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.0f [%.0f-%.0f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    rat = lambda c: "%.2f %s" % (c["ratio_of_medians"], "YES" if c["outside_spread"] else "no")  # noqa: E731
    traced = all("kernel_us" in c for c in res["cells"])
    L = [SECTION, "",
         "`%s` -> `teditl.json` (the traced dispatches one by one: `raw/teditl_scan_kernels.csv`), taken on the kernels and library of commit %s.  1 GiB texts, the pattern cut from the text.  call: ms per call, the host clock around one synchronous call, %d calls after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches after a warm-up.  median [min-max]: the bracket is the run-to-run spread.  A ratio is followed by YES when the medians differ by more than the larger of the two spreads, by no when they lie inside it.  Recorded as measured; nothing is required of these numbers." % (
             res.get("command"), res.get("commit"), res["reps"], res.get("trace_reps", 0)), "",
         "`search_editl` (`text_editl_scan`) with the cut-off (flags = 0) and with every block of every column (`SMARTGPU_EDITL_ALL_BLOCKS`).  A lane owns a run of %d end positions and walks up to m + k bytes before it: the warm-up factor is (%d + m + k) / %d.  W = ceil(m / 32) blocks." % (res["run"], res["run"], res["run"]), "",
         "### Cut-off against all blocks", "",
         "| text | m | k | warm-up | ends | W | cut-off, ms per call | all blocks, ms per call | all / cut | GB/s (call) | cut-off kernel, us | all blocks kernel, us | all / cut | GB/s (kernel) |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        ku = c.get("kernel_us")
        L.append("| %s | %d | %d | %.2f | %d | %d | %s | %s | %s | %.0f | %s | %s | %s | %s |" % (
            c["text"], c["m"], c["k"], c["warm_up_factor"], c["count"], (c["m"] + 31) // 32, fms(c["call_ms"]["cut"]), fms(c["call_ms"]["all"]),
            rat(c["all_over_cut"]), c["gb_per_s_call"], fus(ku["cut"]) if ku else "not measured", fus(ku["all"]) if ku else "not measured",
            rat(c["kernel_all_over_cut"]) if ku else "", "%.0f" % c["gb_per_s_kernel"] if ku else ""))
    L += ["", "### text_editl_scan against text_edit_scan at m = 64, k <= 7", "",
          "The same pattern and text; `text_edit_scan` (`search_edit`) keeps the whole column in two dwords and owns runs of 128 end positions, unchanged from the parent commit.", "",
          "| text | k | search_edit, ms per call | search_editl, ms per call | editl / edit | text_edit_scan, us | text_editl_scan, us | editl / edit |", "|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        if "edit64" in c["call_ms"]:
            ku = c.get("kernel_us")
            L.append("| %s | %d | %s | %s | %s | %s | %s | %s |" % (
                c["text"], c["k"], fms(c["call_ms"]["edit64"]), fms(c["call_ms"]["cut"]), rat(c["cut_over_edit64"]),
                fus(ku["edit64"]) if ku else "not measured", fus(ku["cut"]) if ku else "not measured", rat(c["kernel_cut_over_edit64"]) if ku else ""))
    L += ["", "### text_editl_scan against planes_editl_scan on the same rand4 bytes, packed", "",
          "The same recurrence, run length, P and k; the text from two bit planes by direct loads and the masks from kernel arguments (`psearch_editl`) against the text from LDS rows and the masks from an LDS table (`search_editl`).  bytes / packed is the price of bytes.", "",
          "| m | k | psearch_editl, ms per call | search_editl, ms per call | bytes / packed | planes_editl_scan, us | text_editl_scan, us | bytes / packed |", "|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        if "packed" in c["call_ms"]:
            ku = c.get("kernel_us")
            L.append("| %d | %d | %s | %s | %s | %s | %s | %s |" % (
                c["m"], c["k"], fms(c["call_ms"]["packed"]), fms(c["call_ms"]["cut"]), rat(c["cut_over_packed"]),
                fus(ku["packed"]) if ku else "not measured", fus(ku["cut"]) if ku else "not measured", rat(c["kernel_cut_over_packed"]) if ku else ""))
    L += ["", "### NOT measured", "",
          "The occupancy choice (4 / 4 / 3 workgroups per CU for 2 / 4 / 8 dwords is what the LDS holds; `__launch_bounds__` follows it); the run of %d end positions per lane and the piece of 128 bytes against other lengths; a prefetch of the next piece while the current one is walked; the find form's speed and the host ordering's share in it; the classes calls (the kernels are the same, the host builds another table); the number of active blocks on the device; texts beyond 1 GiB; hardware counters." % res["run"], ""]
    path = os.path.join(os.path.dirname(a.out), "RESULTS.md")
    if not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", "tedit", "RESULTS.md")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tedit", "teditl.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "teditl_probe"))
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
