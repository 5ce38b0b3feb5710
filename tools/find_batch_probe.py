#!/usr/bin/env python3
"""Positions of a pattern set on a byte text, on the GPU: python tools/find_batch_probe.py [--out profiles/coalesce/raw/findbatch_result.json]

1 GiB of rand128, m in MS, one full pass of patterns (find_width(m)) and 200 patterns, all cut from the text.  Numbers
only, nothing is required of them:
  1. call     one find_batch call against the same patterns through K find() calls — the only answer there was before
              the call existed; find() is untouched, so both sides are timed on this build;
  2. kernel   hor_multi_find's time per pass against hor_multi_scan's for the same patterns, range and width: the scan
              side queues the width's plans (smartgpu_coalesce_pass, long passes on) so that they leave as one pass;
              from a `rocprofv3 --kernel-trace` run of its own;
  3. stage    the call over a text with 2^20 planted occurrences (a 1 KiB unit that holds one pattern of the set once,
              tiled to 1 GiB) against the same call over the unplanted text.
Per call: the host clock around one synchronous call, REPS calls after a warm-up, the sides alternating.  Medians with
[min-max]; a ratio counts as a difference only where the medians differ by more than the larger spread.

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails.  `render` writes
the section "Positions of a pattern set" of profiles/coalesce/RESULTS.md from the JSON file."""
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

MS = (16, 32, 64)
N = 1 << 30
REPS, TRACE_REPS = 5, 4
WIDE = 200
UNIT = 1024
SECTION = "## Positions of a pattern set"


def clocked(fn):
    t0 = time.perf_counter()
    got = fn()
    return (time.perf_counter() - t0) * 1e3, got


def patterns(text, m, K):
    """K patterns of m bytes cut from the text at spread positions (rand128: each occurs once, and streams)."""
    step = (N - m - 4096) // K
    return [text.read(1000 + k * step, m) for k in range(K)]


def widths(m):
    import smart_amd
    return (("pass", smart_amd.find_width(m)), ("200", WIDE))


def measure(out):
    import numpy as np
    import smart_amd
    res = {"reps": REPS, "unit": "ms per call (host clock around one synchronous call)", "n": N, "cells": [], "stage": []}
    text = smart_amd.Text.generate(0x5EED0400 + 128, 128, N)
    for m in MS:
        for label, K in widths(m):
            pats = patterns(text, m, K)
            t = {"find_batch": [], "find_each": []}
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                for side in (("find_batch", "find_each") if rep % 2 else ("find_each", "find_batch")):
                    if side == "find_batch":
                        ms, (lists, counts) = clocked(lambda: smart_amd.find_batch(pats, text))
                    else:
                        ms, each = clocked(lambda: [smart_amd.find(P, text) for P in pats])
                    t[side].append(ms)
            assert all(np.array_equal(a, b[0]) for a, b in zip(lists, each)) and int(counts.min()) >= 1, (m, K)
            cell = {"m": m, "set": label, "K": K, "passes": -(-K // smart_amd.find_width(m)), "occurrences": int(counts.sum()),
                    "call_ms": {s: spread(v[1:]) for s, v in t.items()}}
            cell.update(compare(cell["call_ms"]["find_batch"], cell["call_ms"]["find_each"]))
            res["cells"].append(cell)
            print("m=%-2d K=%-3d find_batch %.3f ms  K x find %.3f ms  x%.1f" % (m, K, cell["call_ms"]["find_batch"]["median"], cell["call_ms"]["find_each"]["median"],
                                                                               cell["ratio_of_medians"]), flush=True)
    # the output stage where it matters: 2^20 occurrences of ONE pattern of the set
    rng = np.random.default_rng(7100)
    unit = rng.integers(0, 128, UNIT).astype(np.uint8)
    planted = smart_amd.Text.upload_tiled(unit, N)
    for m in MS:
        K = smart_amd.find_width(m)
        pats = patterns(text, m, K)
        pats[K // 2] = unit[100:100 + m].copy()
        t = {"unplanted": [], "planted": []}
        for rep in range(REPS + 1):
            ms, (_, c0) = clocked(lambda: smart_amd.find_batch(pats, text, cap=1 << 21))
            t["unplanted"].append(ms)
            ms, (lists, c1) = clocked(lambda: smart_amd.find_batch(pats, planted, cap=1 << 21))
            t["planted"].append(ms)
        assert int(c1[K // 2]) == N // UNIT == len(lists[K // 2]) and int(lists[K // 2][0]) == 100 and int(c0[K // 2]) == 0, (m, c1[K // 2])
        cell = {"m": m, "K": K, "occurrences": int(c1.sum()), "call_ms": {s: spread(v[1:]) for s, v in t.items()}}
        cell.update(compare(cell["call_ms"]["unplanted"], cell["call_ms"]["planted"]))
        res["stage"].append(cell)
        print("stage m=%-2d K=%-3d unplanted %.3f ms  2^20 occurrences %.3f ms  x%.2f" % (m, K, cell["call_ms"]["unplanted"]["median"], cell["call_ms"]["planted"]["median"],
                                                                                         cell["ratio_of_medians"]), flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per m, TRACE_REPS + 1 times a find_batch of one full pass, and the same patterns as
    plans queued into one shared pass of the scan."""
    import smart_amd
    from smart_amd import engine
    engine.text_sampling(-1)
    text = smart_amd.Text.generate(0x5EED0400 + 128, 128, N)
    engine.coalesce_sample(0)       # the passes read the text itself, as hor_multi_find does
    engine.coalesce_pass(engine.PASS_MAX)
    engine.coalesce_long(0)
    plan = []
    for m in MS:
        K = min(smart_amd.find_width(m), engine.long_width(m))  # the same width on both sides
        pats = patterns(text, m, K)
        plans = [smart_amd.Plan("hor", P) for P in pats]
        for rep in range(TRACE_REPS + 1):
            _, counts = smart_amd.find_batch(pats, text)
            for pl in plans:
                pl.reset()
            engine.device_sync(0)
            for pl in plans:
                pl.launch(text)
            engine.device_sync(0)
            assert [pl.result(0)[0] for pl in plans] == counts.tolist(), m
            plan.append([m, K, rep])
        for pl in plans:
            pl.free()
    with open(plan_out, "w") as f:
        json.dump(plan, f)


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "findbatch_trace"), os.path.join(a.scratch, "findbatch_plan.json")
    steps = [
        ("measure", ["timeout", "-k", "10", "420"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "findbatch_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if "hor_multi_find" in r["Kernel_Name"] or "hor_multi_scan" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    per = {}
    with open(os.path.join(os.path.dirname(a.out), "findbatch_kernels.csv"), "w") as f:
        f.write("m,K,rep,kernel,us\n")
        at = 0
        for m, K, rep in launches:
            # a repetition: one hor_multi_find, then the scan's pass (or passes, should the queue have split it)
            assert "hor_multi_find" in rows[at]["Kernel_Name"], (rows[at]["Kernel_Name"], m, rep)
            us = (int(rows[at]["End_Timestamp"]) - int(rows[at]["Start_Timestamp"])) / 1e3
            f.write("%d,%d,%d,hor_multi_find,%.3f\n" % (m, K, rep, us))
            at += 1
            scan_us, scans = 0.0, 0
            while at < len(rows) and "hor_multi_scan" in rows[at]["Kernel_Name"]:
                one = (int(rows[at]["End_Timestamp"]) - int(rows[at]["Start_Timestamp"])) / 1e3
                f.write("%d,%d,%d,hor_multi_scan,%.3f\n" % (m, K, rep, one))
                scan_us, scans, at = scan_us + one, scans + 1, at + 1
            if rep:
                per.setdefault((m, "find"), []).append(us)
                per.setdefault((m, "scan"), []).append(scan_us)
                per.setdefault((m, "scans"), []).append(scans)
        assert at == len(rows), (at, len(rows))
    res["kernel"] = []
    for m, K, rep in launches:
        if rep == 0:
            cell = {"m": m, "K": K, "scan_kernels_per_rep": max(per[(m, "scans")]), "kernel_us": {"hor_multi_find": spread(per[(m, "find")]), "hor_multi_scan": spread(per[(m, "scan")])}}
            cell.update(compare(cell["kernel_us"]["hor_multi_scan"], cell["kernel_us"]["hor_multi_find"]))
            res["kernel"].append(cell)
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/find_batch_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def render(a):
    res = json.load(open(a.out))
    fms = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.0f [%.0f-%.0f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    yes = lambda c: "YES" if c["outside_spread"] else "no"  # noqa: E731
    L = [SECTION, "",
         "`%s` -> `raw/%s` (the traced dispatches one by one: `raw/findbatch_kernels.csv`), taken on the kernels and library of commit %s.  1 GiB of rand128, the patterns cut from the text.  call: ms per call, the host clock around one synchronous call, %d calls after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d repetitions after a warm-up.  median [min-max]: the bracket is the run-to-run spread.  outside: the medians differ by more than the larger of the two spreads.  Recorded as measured; nothing is required of these numbers and nothing was tuned toward them." % (
             res.get("command", "python tools/find_batch_probe.py"), os.path.basename(a.out), res.get("commit", "?"), res["reps"], res.get("trace_reps", 0)), "",
         "### One find_batch call against K find() calls", "",
         "`find()` (an EPSM plan, a `hipMalloc`, a whole `packed_find` pass and a host sort per pattern) was the only way to the positions of a set; it is untouched, so both sides ran on this build.  find_batch: staging, the passes, one copy, the host ordering.", "",
         "| m | set | K | passes | occurrences | find_batch, ms per call | K x find, ms | K x find / find_batch | outside |", "|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        L.append("| %d | %s | %d | %d | %d | %s | %s | %.1f | %s |" % (c["m"], c["set"], c["K"], c["passes"], c["occurrences"], fms(c["call_ms"]["find_batch"]), fms(c["call_ms"]["find_each"]),
                                                                     c["ratio_of_medians"], yes(c)))
    L += ["", "### The ceiling: hor_multi_find per pass against hor_multi_scan", "",
          "The same patterns, range and width: the find's pass of a call, and the scan's pass of as many queued `Plan.launch` calls (long passes on, the sample off: both read the text itself).  `scans` says how many scan kernels the queue sent per repetition; their times are added.", ""]
    if res.get("kernel"):
        L += ["| m | K | hor_multi_find, us | hor_multi_scan, us | scans | find / scan | outside |", "|---|---|---|---|---|---|---|"]
        for c in res["kernel"]:
            L.append("| %d | %d | %s | %s | %d | %.2f | %s |" % (c["m"], c["K"], fus(c["kernel_us"]["hor_multi_find"]), fus(c["kernel_us"]["hor_multi_scan"]), c["scan_kernels_per_rep"],
                                                               c["ratio_of_medians"], yes(c)))
    else:
        L += ["Not measured: the kernel trace was not taken."]
    L += ["", "### The output stage at 2^20 occurrences", "",
          "One full pass; one pattern of the set is planted once in a 1 KiB unit that is tiled to 1 GiB (2^20 occurrences, about sixteen per tile), against the same call over the rand128 text where that pattern does not occur.  The planted side also copies 8 MiB of entries to the host and orders them.", "",
          "| m | K | occurrences | unplanted, ms per call | planted, ms per call | planted / unplanted | outside |", "|---|---|---|---|---|---|---|"]
    for c in res["stage"]:
        L.append("| %d | %d | %d | %s | %s | %.2f | %s |" % (c["m"], c["K"], c["occurrences"], fms(c["call_ms"]["unplanted"]), fms(c["call_ms"]["planted"]), c["ratio_of_medians"], yes(c)))
    L += ["", "### NOT measured", "",
          "Occupancy choices (the scan's four or five workgroups per CU were taken over, none swept for this kernel); other stage sizes than 128 entries, and with them other pass widths; texts where occurrences are dense (every start, small alphabets: the overflow path's atomics) beyond the one planted case above; the split of a call between staging, kernel, copy and host ordering; sets of several passes against the scan's; m beyond 64; hardware counters.", ""]
    path = os.path.join(ROOT, "profiles", "coalesce", "RESULTS.md")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coalesce", "raw", "findbatch_result.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "find_batch_probe"))
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
