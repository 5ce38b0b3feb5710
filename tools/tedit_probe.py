#!/usr/bin/env python3
"""Edit distance on byte texts, on the GPU: python tools/tedit_probe.py [--out profiles/tedit/tedit.json]

1 GiB texts, m in MS, k in KS, the pattern cut from the text.  Numbers only, nothing is required of them:
  1. texts        search_edit on rand4, rand128 and the English corpus tiled to 1 GiB;
  2. packed       psearch_edit on the packed text of the same rand4 bytes, the same P and k: the same recurrence with the
                  text and mask paths swapped — the ratio is the price of bytes;
  3. conflicts    rand256 (nearly all-distinct mask lookups in a wave) against a text of ONE value (all-broadcast lookups)
                  at the same m and k, the pattern m times that value.
  4. stride       (a step of its own: `stride --variant smart_amd/csrc/libsmartgpu_<name>.so`) the product's padded row of
                  132 bytes against a `tools/build_variant.sh <name> -DSMARTGPU_TEDIT_ROW_PAD=0` build on rand256, both
                  libraries in one process, the sides alternating; written to tedit_stride.json beside the --out file.
Per call: the host clock around one synchronous call, REPS calls after a warm-up.  Per kernel: a `rocprofv3 --kernel-trace`
run of its own, TRACE_REPS dispatches after a warm-up.  Medians with [min-max].

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails.  `render` writes
profiles/tedit/RESULTS.md from the JSON file."""
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
KS = (0, 3, 7)
N = 1 << 30
REPS, TRACE_REPS = 7, 5
RUN = 128  # tedit_host.hpp kTEditRun
TEXTS = ("rand4", "rand128", "english", "rand256", "one_value")


def make_text(name):
    import numpy as np
    import smart_amd
    from smart_amd import corpus
    if name.startswith("rand"):
        sigma = int(name[4:])
        return smart_amd.Text.generate(0x5EED0400 + sigma, sigma, N)
    if name == "english":
        return smart_amd.Text.upload_tiled(corpus.english_unit(), N)
    return smart_amd.Text.upload_tiled(np.full(4096, ord("a"), dtype=np.uint8), N)


def sides(name, text):
    """[(side, call(P, k))] for a text: search_edit, and on rand4 psearch_edit on the same bytes packed."""
    import smart_amd
    out = [("search_edit", lambda P, k: smart_amd.search_edit(P, text, k))]
    pt = None
    if name == "rand4":
        pt = smart_amd.PackedText.pack(text)
        out.append(("psearch_edit", lambda P, k: smart_amd.psearch_edit(P, pt, k)[0]))
    return out, pt


def clocked(fn):
    t0 = time.perf_counter()
    got = fn()
    return (time.perf_counter() - t0) * 1e3, got


def measure(out):
    res = {"reps": REPS, "unit": "ms per call (host clock around one synchronous call)", "run": RUN, "n": N, "cells": []}
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
                assert len(set(counts.values())) == 1 and counts["search_edit"] >= 1, (name, m, k, counts)  # both kernels count the same ends
                cell = {"text": name, "m": m, "k": k, "count": counts["search_edit"], "warm_up_factor": (RUN + m + k) / RUN,
                        "call_ms": {s: spread(v[1:]) for s, v in t.items()}}
                cell["gb_per_s_call"] = N / (cell["call_ms"]["search_edit"]["median"] * 1e-3) / 1e9
                res["cells"].append(cell)
                print("%-9s m=%-2d k=%d %s  %.0f GB/s, %d ends" % (name, m, k, "  ".join("%s %.3f ms" % (s, v["median"]) for s, v in cell["call_ms"].items()),
                                                                 cell["gb_per_s_call"], cell["count"]), flush=True)
        if pt:
            pt.free()
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


def stride(out, variant):
    """The product library against a variant build of another row stride, per call, on rand256 at k = 3."""
    from smart_amd import engine
    libs = [("padded", engine.LIB_PATH), ("variant", os.path.abspath(variant))]
    texts = {}
    for side, path in libs:
        engine.use_library(path)
        texts[side] = make_text("rand256")
    res = {"reps": REPS, "variant": os.path.basename(variant), "text": "rand256", "cells": []}
    for m in MS:
        engine.use_library(libs[0][1])  # (a text is read through the library that made it)
        P = texts["padded"].read(N // 3 + 17, m)
        for k in (3,):
            t, counts = {side: [] for side, _ in libs}, {}
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                for side, path in (libs if rep % 2 else libs[::-1]):
                    engine.use_library(path)
                    ms, counts[side] = clocked(lambda: engine.search_edit(P, texts[side], k))
                    t[side].append(ms)
            assert counts["padded"] == counts["variant"] >= 1, (m, k, counts)
            cell = {"m": m, "k": k, "count": counts["padded"], "call_ms": {side: spread(v[1:]) for side, v in t.items()}}
            cell.update(compare(cell["call_ms"]["padded"], cell["call_ms"]["variant"]))
            res["cells"].append(cell)
            print("rand256 m=%-2d k=%d padded %.3f ms  variant %.3f ms  x%.2f outside=%s" % (
                m, k, cell["call_ms"]["padded"]["median"], cell["call_ms"]["variant"]["median"], cell["ratio_of_medians"], cell["outside_spread"]), flush=True)
    for side, path in libs:
        engine.use_library(path)
        texts[side].free()
    with open(os.path.join(os.path.dirname(out), "tedit_stride.json"), "w") as f:
        json.dump(res, f, indent=1)


KERNEL_OF = {"search_edit": "text_edit_scan", "psearch_edit": "planes_edit_scan"}


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "tedit_trace"), os.path.join(a.scratch, "tedit_plan.json")
    steps = [
        ("measure", ["timeout", "-k", "10", "300"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "tedit_" + name.replace(" ", "_") + ".log"), "w") as log:
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
    with open(os.path.join(raw, "tedit_scan_kernels.csv"), "w") as f:
        f.write("text,m,k,side,rep,kernel,us\n")
        for r, (name, m, k, side, rep) in zip(rows, launches):
            assert KERNEL_OF[side] in r["Kernel_Name"], (r["Kernel_Name"], name, m, k, side, rep)
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            f.write("%s,%d,%d,%s,%d,%s,%.3f\n" % (name, m, k, side, rep, KERNEL_OF[side], us))
            if rep:
                per.setdefault((name, m, k, side), []).append(us)
    for cell in res["cells"]:
        cell["kernel_us"] = {s: spread(per[(cell["text"], cell["m"], cell["k"], s)]) for s in cell["call_ms"]}
        cell["gb_per_s_kernel"] = N / (cell["kernel_us"]["search_edit"]["median"] * 1e-6) / 1e9
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/tedit_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def render(a):
    res = json.load(open(a.out))
    cells = {(c["text"], c["m"], c["k"]): c for c in res["cells"]}
    fms = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.0f [%.0f-%.0f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    traced = all("kernel_us" in c for c in res["cells"])
    L = ["# Edit distance on byte texts (text_edit_scan)", "",
         "`%s` -> `tedit.json` (the traced dispatches one by one: `raw/tedit_scan_kernels.csv`), taken on the kernels and library of commit %s.  1 GiB texts.  call: ms per call, the host clock around one synchronous `search_edit`, %d calls after a warm-up; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches after a warm-up.  median [min-max]: the bracket is the run-to-run spread.  outside: the medians differ by more than the larger of the two spreads.  Recorded as measured; nothing is required of these numbers." % (
             res.get("command"), res.get("commit"), res["reps"], res.get("trace_reps", 0)), "",
         "A lane owns %d end positions and walks up to m + k bytes before them: the warm-up factor is (%d + m + k) / %d." % (res["run"], res["run"], res["run"]), "",
         "## 1. Texts", "",
         "| text | m | k | warm-up | ends | search_edit, ms per call | GB/s (call) | text_edit_scan, us | GB/s (kernel) |", "|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        if c["text"] in ("rand4", "rand128", "english"):
            L.append("| %s | %d | %d | %.2f | %d | %s | %.0f | %s | %s |" % (
                c["text"], c["m"], c["k"], c["warm_up_factor"], c["count"], fms(c["call_ms"]["search_edit"]), c["gb_per_s_call"],
                fus(c["kernel_us"]["search_edit"]) if traced else "not measured", "%.0f" % c["gb_per_s_kernel"] if traced else ""))
    L += ["", "## 2. Against psearch_edit on the same rand4 bytes, packed", "",
          "The same recurrence, P and k; the text from two bit planes by direct loads and the mask from kernel arguments (`planes_edit_scan`) against the text from an LDS tile and the mask from an LDS table (`text_edit_scan`).  bytes / packed is the price of bytes.", "",
          "| m | k | psearch_edit, ms per call | search_edit, ms per call | bytes / packed | outside | planes_edit_scan, us | text_edit_scan, us | bytes / packed | outside |", "|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        if c["text"] == "rand4":
            call = compare(c["call_ms"]["psearch_edit"], c["call_ms"]["search_edit"])
            kern = compare(c["kernel_us"]["psearch_edit"], c["kernel_us"]["search_edit"]) if traced else None
            L.append("| %d | %d | %s | %s | %.2f | %s | %s | %s | %s | %s |" % (
                c["m"], c["k"], fms(c["call_ms"]["psearch_edit"]), fms(c["call_ms"]["search_edit"]), call["ratio_of_medians"], "YES" if call["outside_spread"] else "no",
                fus(c["kernel_us"]["psearch_edit"]) if traced else "not measured", fus(c["kernel_us"]["search_edit"]) if traced else "not measured",
                "%.2f" % kern["ratio_of_medians"] if kern else "", ("YES" if kern["outside_spread"] else "no") if kern else ""))
    L += ["", "## 3. Mask-lookup conflicts: rand256 against a one-value text", "",
          "On rand256 the 64 lanes of a wave read nearly all-distinct entries of the LDS mask table per step (bank conflicts as the text deals them); on a text of one value every lane reads the same entry (a broadcast).  Same m and k; the patterns differ (cut from the text), which the recurrence does not see in its instruction count.", "",
          "| m | k | one value, ms per call | rand256, ms per call | rand256 / one value | outside | one value, us | rand256, us | rand256 / one value | outside |", "|---|---|---|---|---|---|---|---|---|---|"]
    for m in MS:
        for k in KS:
            if ("rand256", m, k) not in cells or ("one_value", m, k) not in cells:
                continue
            a1, b1 = cells[("one_value", m, k)], cells[("rand256", m, k)]
            call = compare(a1["call_ms"]["search_edit"], b1["call_ms"]["search_edit"])
            kern = compare(a1["kernel_us"]["search_edit"], b1["kernel_us"]["search_edit"]) if traced else None
            L.append("| %d | %d | %s | %s | %.2f | %s | %s | %s | %s | %s |" % (
                m, k, fms(a1["call_ms"]["search_edit"]), fms(b1["call_ms"]["search_edit"]), call["ratio_of_medians"], "YES" if call["outside_spread"] else "no",
                fus(a1["kernel_us"]["search_edit"]) if traced else "not measured", fus(b1["kernel_us"]["search_edit"]) if traced else "not measured",
                "%.2f" % kern["ratio_of_medians"] if kern else "", ("YES" if kern["outside_spread"] else "no") if kern else ""))
    stride_json = os.path.join(os.path.dirname(a.out), "tedit_stride.json")
    if os.path.exists(stride_json):
        st = json.load(open(stride_json))
        L += ["", "## 4. The padded row against an unpadded one", "",
              "The product (rows of 132 bytes: the 32 lanes of a `ds_read_b32` group on 32 banks) against a `tools/build_variant.sh` build with `-DSMARTGPU_TEDIT_ROW_PAD=0` (rows of 128 bytes: a group's lanes on ONE bank), %s, both libraries in one process, the sides alternating, ms per call by the host clock, %d calls after a warm-up.  No kernel trace was taken of the variant." % (st["text"], st["reps"]), "",
              "| m | k | padded (132), ms per call | unpadded (128), ms per call | unpadded / padded | outside |", "|---|---|---|---|---|---|"]
        for c in st["cells"]:
            L.append("| %d | %d | %s | %s | %.2f | %s |" % (c["m"], c["k"], fms(c["call_ms"]["padded"]), fms(c["call_ms"]["variant"]), c["ratio_of_medians"], "YES" if c["outside_spread"] else "no"))
    L += ["", "## NOT measured", "",
          ("Four" if os.path.exists(stride_json) else "The padded row of 132 bytes against an unpadded one (a `tools/build_variant.sh` build); four") + " workgroups per CU and `__launch_bounds__(256, 4)` against other occupancies; the run of %d end positions per lane; a double-buffered tile; the find form's speed and the host ordering's share in it; the classes calls (the kernels are the same, the host builds another table); texts beyond 1 GiB; hardware counters (LDS bank conflicts are inferred from section 3's times, not counted)." % res["run"], ""]
    path = os.path.join(os.path.dirname(a.out), "RESULTS.md")
    with open(path, "w") as f:
        f.write("\n".join(L))
    print("rendered " + path)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "render", "stride"))
    ap.add_argument("--variant", help="stride: the variant library (tools/build_variant.sh)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tedit", "tedit.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "tedit_probe"))
    ap.add_argument("--commit", help="the commit the numbers are taken on (default: git rev-parse HEAD)")
    a = ap.parse_args()
    a.out, a.scratch = os.path.abspath(a.out), os.path.abspath(a.scratch)
    if a.step == "measure":
        return measure(a.out)
    if a.step == "workload":
        return workload(a.out)
    if a.step == "render":
        return render(a)
    if a.step == "stride":
        return stride(a.out, a.variant)
    return driver(a) or render(a)


if __name__ == "__main__":
    sys.exit(main())
