#!/usr/bin/env python3
"""Edit distance on packed texts, on the GPU: python tools/edit_probe.py [--out profiles/packed/packed_edit.json]

1 Gi symbols of rand4 and of rand2.  Numbers only, nothing is required of them:
  psearch_edit with k = 0, 1, 3, 7, m in MS, the pattern cut from the text, and next to it psearch_mis of the same pattern and
  k — the nearest question the library already answers (start positions within Hamming distance k; the edit call answers
  END positions within edit distance k, a superset shifted by m - 1) — per call and per kernel, and symbols per second.

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails:
  1. `measure`   call times: the device's stream events around BATCH back-to-back calls, REPS repetitions after a warm-up, the
                 sides alternating inside every repetition;
  2. `rocprofv3 --kernel-trace --stats -- ... workload`   kernel times, a run of its own.
`render` writes the "Edit distance" section of profiles/packed/RESULTS.md from the JSON file (the method is
tools/mis_probe.py's)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sets_probe import commit, compare, make_text, rows_of, spread, timed  # noqa: E402

MS = (8, 16, 20, 32, 33, 64)
KS = (0, 1, 3, 7)
BATCH, REPS, TRACE_REPS = 20, 10, 10
TEXTS = (("rand4_1Gi", 4, 1 << 30), ("rand2_1Gi", 2, 1 << 30))
RUN = 128  # pedit.hpp kEditRun: end positions a lane owns; it walks up to m + k symbols before them


def measure(out):
    import smart_amd
    res = {"batch": BATCH, "reps": REPS, "unit": "ms per call (device events around %d back-to-back calls)" % BATCH, "run": RUN, "cells": []}
    for name, sigma, n in TEXTS:
        text, pt = make_text(sigma, n)
        for m in MS:
            P = text.read(n // 3 + 17, m)
            exact = smart_amd.psearch(P, pt)[0]
            t = {(side, k): [] for side in ("edit", "mis") for k in KS}
            counts = {}
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                sides = sorted(t)
                for side, k in (sides if rep % 2 else sides[::-1]):
                    if side == "edit":
                        ms, got = timed(lambda: smart_amd.psearch_edit(P, pt, k)[0])
                        assert got >= exact and (k or got == exact), (name, m, k, got, exact)
                    else:
                        ms, got = timed(lambda: smart_amd.psearch_mis(P, pt, k)[0])
                        assert got >= exact and (k or got == exact), (name, m, k, got, exact)
                    counts[(side, k)] = got
                    t[(side, k)].append(ms)
            for k in KS:
                assert counts[("edit", k)] >= counts[("mis", k)], (name, m, k, counts)  # every Hamming occurrence ends an edit occurrence
                e, h = spread(t[("edit", k)][1:]), spread(t[("mis", k)][1:])
                cell = {"text": name, "n": n, "m": m, "k": k, "count": counts[("edit", k)], "count_mis": counts[("mis", k)],
                        "psearch_edit_ms": e, "psearch_mis_ms": h, "warm_up_factor": (RUN + m + k) / RUN,
                        "gsymbols_per_s_call": n / (e["median"] * 1e-3) / 1e9}
                cell.update(compare(h, e))
                res["cells"].append(cell)
                print("%-10s m=%-3d k=%d edit %.4f ms (%.1f Gsym/s, %d)  mis %.4f ms (%d)  x%.2f outside=%s" % (
                    name, m, k, e["median"], cell["gsymbols_per_s_call"], cell["count"], h["median"], cell["count_mis"],
                    cell["ratio_of_medians"], cell["outside_spread"]), flush=True)
        pt.free()
        text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per text, m and k, planes_edit_scan and planes_mis_scan, TRACE_REPS + 1 times."""
    import smart_amd
    plan = []
    for name, sigma, n in TEXTS:
        text, pt = make_text(sigma, n)
        for m in MS:
            P = text.read(n // 3 + 17, m)
            for rep in range(TRACE_REPS + 1):
                for k in KS:
                    smart_amd.psearch_edit(P, pt, k)
                    plan.append([name, m, k, "edit", rep])
                    smart_amd.psearch_mis(P, pt, k)
                    plan.append([name, m, k, "mis", rep])
        pt.free()
        text.free()
    with open(plan_out, "w") as f:
        json.dump(plan, f)


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "edit_trace"), os.path.join(a.scratch, "edit_plan.json")
    steps = [
        ("measure", ["timeout", "-k", "10", "420"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "edit_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if "planes_edit_scan" in r["Kernel_Name"] or "planes_mis_scan" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    for r, (name, m, k, kind, rep) in zip(rows, launches):
        assert ("planes_edit_scan" in r["Kernel_Name"]) == (kind == "edit"), (r["Kernel_Name"], name, m, k, kind, rep)
        if rep:
            per.setdefault((name, m, k, kind), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for cell in res["cells"]:
        e, h = spread(per[(cell["text"], cell["m"], cell["k"], "edit")]), spread(per[(cell["text"], cell["m"], cell["k"], "mis")])
        cell["kernel_us"] = {"planes_edit_scan": e, "planes_mis_scan": h}
        cell["kernel_us"].update(compare(h, e))
        cell["gsymbols_per_s_kernel"] = cell["n"] / (e["median"] * 1e-6) / 1e9
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/edit_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def render(a):
    """The "Edit distance" section of RESULTS.md, appended (or replaced where it stands)."""
    res = json.load(open(a.out))
    fmt = lambda v: "%.4f [%.4f-%.4f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.1f [%.1f-%.1f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    note = lambda t: " (possibly flattered)" if t.startswith("rand2") else ""  # noqa: E731
    L = ["## Edit distance", "",
         "`%s` -> `packed_edit.json`, taken on the kernels and library of commit %s.  1 Gi symbols; call: ms per call from the device's stream events around %d back-to-back calls, %d repetitions after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches per side after a warm-up.  median [min-max].  outside: the medians differ by more than the larger of the two spreads.  The rand2 planes (128 MiB) are of Infinity-Cache size: possibly flattered." % (
             res.get("command"), res.get("commit"), res["batch"], res["reps"], res.get("trace_reps", 0)), "",
         "`psearch_edit` (END positions within edit distance k, `planes_edit_scan`) next to `psearch_mis` of the same pattern and k (start positions within Hamming distance k, `planes_mis_scan`): the nearest question the library already answers, not the same one.  A lane owns a run of %d end positions and walks up to m + k symbols before it: the warm-up factor is (%d + m + k) / %d.  Recorded as measured; nothing is required of it." % (res["run"], res["run"], res["run"]), "",
         "| text | m | k | warm-up | occurrences (edit / mis) | psearch_mis, ms | psearch_edit, ms | edit / mis | outside | Gsym/s (call) | planes_mis_scan, us | planes_edit_scan, us | edit / mis | outside | Gsym/s (kernel) |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        k = c.get("kernel_us")
        L.append("| %s%s | %d | %d | %.2f | %d / %d | %s | %s | %.2f | %s | %.1f | %s | %s | %s | %s | %s |" % (
            c["text"], note(c["text"]), c["m"], c["k"], c["warm_up_factor"], c["count"], c["count_mis"], fmt(c["psearch_mis_ms"]), fmt(c["psearch_edit_ms"]),
            c["ratio_of_medians"], "YES" if c["outside_spread"] else "no", c["gsymbols_per_s_call"],
            fus(k["planes_mis_scan"]) if k else "not measured", fus(k["planes_edit_scan"]) if k else "not measured",
            "%.2f" % k["ratio_of_medians"] if k else "", ("YES" if k["outside_spread"] else "no") if k else "",
            "%.1f" % c["gsymbols_per_s_kernel"] if k else ""))
    L += ["", "Choices that are NOT measured: the run of %d end positions per lane (a longer run lowers the warm-up factor and spreads a wave's loads over more cache lines), 8 workgroups per CU and `__launch_bounds__(256, 8)`, one run per lane and trip (no unrolling across runs), the code's selection of the mask by `v_cndmask`; the find form's speed; texts beyond 1 Gi symbols." % res["run"]]
    path = os.path.join(os.path.dirname(a.out), "RESULTS.md")
    if not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", "packed", "RESULTS.md")
    text = open(path).read()
    at = text.find("\n## Edit distance")
    if at >= 0:
        end = text.find("\n## ", at + 1)
        text = text[:at] + (text[end:] if end >= 0 else "\n")
    text = text.rstrip("\n") + "\n\n" + "\n".join(L) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("rendered the Edit distance section of " + path)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_edit.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "edit_probe"))
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
