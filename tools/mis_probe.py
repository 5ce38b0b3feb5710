#!/usr/bin/env python3
"""Mismatches on packed texts, on the GPU: python tools/mis_probe.py [--out profiles/packed/packed_mis.json]

1 Gi symbols of rand4 and of rand2.  Numbers only; ONE cell carries a requirement (2, k = 1):
  (1) psearch_mis with k = 0, 1, 3, 7 against psearch of the same pattern cut from the text, m in MS: the price of the counter;
  (2) rand4, m = 16: ONE psearch_mis call with k = 1 against the 16 psearch_sets calls, one full-set position each, that give
      the same answer today (counting only, no host union: this flatters the alternative); k = 2 against the 120 placements
      of two full-set positions, a sample of PAIRS_TIMED of them timed and scaled;
  (3) pfind_mis, m = 20, k = 2, rand4, against pfind_sets of a one-N pattern of the same length.

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails:
  1. `measure`   call times: the device's stream events around BATCH back-to-back calls, REPS repetitions after a warm-up, the
                 sides alternating inside every repetition;
  2. `rocprofv3 --kernel-trace --stats -- ... workload`   kernel times of (1), a run of its own.
`asm --parent-asm A.s --new-asm B.s` needs no GPU: it stores `tools/asm_stats.py --diff` of the parent's `k_planes` assembly
against this one, and the new kernels' counts, in the JSON file (keys `asm_diff`, `asm_new`); the driver keeps both keys.
`render` writes the "Mismatches" section of profiles/packed/RESULTS.md from the JSON file (the method is tools/sets_probe.py's)."""
import argparse
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sets_probe import commit, compare, make_text, rows_of, singletons, spread, timed  # noqa: E402

MS = (8, 16, 20, 32, 64, 256)
KS = (0, 1, 3, 7)
BATCH, REPS, TRACE_REPS = 20, 10, 10
TEXTS = (("rand4_1Gi", 4, 1 << 30), ("rand2_1Gi", 2, 1 << 30))
PLACE_M, PAIRS_TIMED = 16, 12
FIND_M, FIND_K = 20, 2


def measure(out):
    import numpy as np
    import smart_amd
    res = {"batch": BATCH, "reps": REPS, "unit": "ms per call (device events around %d back-to-back calls)" % BATCH,
           "counter": [], "placements": [], "find": []}
    for name, sigma, n in TEXTS:
        text, pt = make_text(sigma, n)
        sym = pt.symbols()
        for m in MS:
            P = text.read(n // 3 + 17, m)
            want = smart_amd.psearch(P, pt)[0]
            t = {"exact": []}
            t.update({k: [] for k in KS})
            counts = {}
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                sides = ["exact"] + list(KS)
                for side in (sides if rep % 2 else sides[::-1]):
                    if side == "exact":
                        ms, got = timed(lambda: smart_amd.psearch(P, pt)[0])
                        assert got == want
                    else:
                        ms, got = timed(lambda: smart_amd.psearch_mis(P, pt, side)[0])
                        assert got >= want and (side or got == want), (name, m, side, got, want)
                        counts[side] = got
                    t[side].append(ms)
            e = spread(t["exact"][1:])
            for k in KS:
                s = spread(t[k][1:])
                cell = {"text": name, "m": m, "k": k, "count": counts[k], "psearch_ms": e, "psearch_mis_ms": s}
                cell.update(compare(e, s))
                res["counter"].append(cell)
                print("%-10s m=%-4d k=%d exact %.4f  mis %.4f  x%.3f outside=%s (count %d)" % (
                    name, m, k, e["median"], s["median"], cell["ratio_of_medians"], cell["outside_spread"], counts[k]), flush=True)
        if sigma == 4:
            # (2) one call against the placements of full sets
            P = text.read(n // 3 + 17, PLACE_M)
            full = (1 << len(sym)) - 1
            for k, places in ((1, [(j,) for j in range(PLACE_M)]), (2, list(itertools.combinations(range(PLACE_M), 2)))):
                timed_places = places if k == 1 else places[::len(places) // PAIRS_TIMED][:PAIRS_TIMED]
                sets = []
                for pl in timed_places:
                    S = singletons(P, sym)
                    S[list(pl)] = full
                    sets.append(S)
                one, many = [], []
                for rep in range(REPS + 1):
                    for side in (("one", "many") if rep % 2 else ("many", "one")):
                        if side == "one":
                            ms, got = timed(lambda: smart_amd.psearch_mis(P, pt, k)[0])
                            one.append(ms)
                        else:
                            tot = 0.0
                            for S in sets:
                                ms, c = timed(lambda: smart_amd.psearch_sets(S, pt)[0])
                                assert c <= got if rep else True
                                tot += ms
                            many.append(tot * len(places) / len(sets))
                o, a = spread(one[1:]), spread(many[1:])
                cell = {"text": name, "m": PLACE_M, "k": k, "placements": len(places), "placements_timed": len(sets), "count": got,
                        "psearch_mis_ms": o, "psearch_sets_all_placements_ms": a, "required": k == 1}
                cell.update(compare(o, a))
                cell["one_call_faster_outside_spread"] = bool(cell["outside_spread"] and a["median"] > o["median"])
                res["placements"].append(cell)
                print("%-10s m=%d k=%d: one psearch_mis call %.4f ms, %d placements by psearch_sets %.4f ms: x%.2f outside=%s" % (
                    name, PLACE_M, k, o["median"], len(places), a["median"], cell["ratio_of_medians"], cell["outside_spread"]), flush=True)
            # (3) the find
            P = text.read(n // 3 + 17, FIND_M)
            S = singletons(P, sym)
            S[FIND_M // 2] = full
            fm, fs = [], []
            for rep in range(REPS + 1):
                for side in (("mis", "sets") if rep % 2 else ("sets", "mis")):
                    if side == "mis":
                        ms, got = timed(lambda: smart_amd.pfind_mis(P, pt, FIND_K)[2])
                        fm.append(ms)
                    else:
                        ms, gots = timed(lambda: smart_amd.pfind_sets(S, pt)[1])
                        fs.append(ms)
            a, b = spread(fs[1:]), spread(fm[1:])
            cell = {"text": name, "m": FIND_M, "k": FIND_K, "count": got, "count_one_N": gots, "pfind_sets_ms": a, "pfind_mis_ms": b}
            cell.update(compare(a, b))
            res["find"].append(cell)
            print("%-10s find m=%d k=%d: pfind_mis %.4f ms (%d), pfind_sets one N %.4f ms (%d): x%.3f" % (
                name, FIND_M, FIND_K, b["median"], got, a["median"], gots, cell["ratio_of_medians"]), flush=True)
        pt.free()
        text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per text and m, planes_scan and planes_mis_scan with k in KS, TRACE_REPS + 1 times."""
    import smart_amd
    plan = []
    for name, sigma, n in TEXTS:
        text, pt = make_text(sigma, n)
        for m in MS:
            P = text.read(n // 3 + 17, m)
            for rep in range(TRACE_REPS + 1):
                smart_amd.psearch(P, pt)
                plan.append([name, m, "exact", rep])
                for k in KS:
                    smart_amd.psearch_mis(P, pt, k)
                    plan.append([name, m, k, rep])
        pt.free()
        text.free()
    with open(plan_out, "w") as f:
        json.dump(plan, f)


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "mis_trace"), os.path.join(a.scratch, "mis_plan.json")
    kept = {}
    if os.path.exists(a.out):  # part (4) is taken without a GPU (`asm`): measure writes the file anew
        kept = {k: v for k, v in json.load(open(a.out)).items() if k in ("asm_diff", "asm_new")}
    steps = [
        ("measure", ["timeout", "-k", "10", "420"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "mis_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if "planes_scan" in r["Kernel_Name"] or "planes_mis_scan" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    for r, (name, m, kind, rep) in zip(rows, launches):
        assert ("planes_mis_scan" in r["Kernel_Name"]) == (kind != "exact"), (r["Kernel_Name"], name, m, kind, rep)
        if rep:
            per.setdefault((name, m, kind), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for cell in res["counter"]:
        e, s = spread(per[(cell["text"], cell["m"], "exact")]), spread(per[(cell["text"], cell["m"], cell["k"])])
        cell["kernel_us"] = {"planes_scan": e, "planes_mis_scan": s}
        cell["kernel_us"].update(compare(e, s))
    res.update(kept)
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/mis_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def asm(a):
    """Part (4), on the build machine: the assembly diff and the new kernels' counts into the JSON file."""
    stats = [sys.executable, os.path.join(ROOT, "tools", "asm_stats.py")]
    diff = subprocess.check_output(stats + ["--diff", a.parent_asm, a.new_asm], text=True).splitlines()
    new = [l[:118] for l in subprocess.check_output(stats + [a.new_asm], text=True).splitlines() if "planes_mis_" in l]
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res["asm_diff"], res["asm_new"] = [l[:118] for l in diff], new
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("stored asm_diff (%d lines) and asm_new (%d kernels) in %s" % (len(diff), len(new), a.out))
    return 0


def render(a):
    """The "Mismatches" section of RESULTS.md, appended (or replaced where it stands)."""
    res = json.load(open(a.out))
    fmt = lambda v: "%.4f [%.4f-%.4f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.1f [%.1f-%.1f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    note = lambda t: " (possibly flattered)" if t.startswith("rand2") else ""  # noqa: E731
    L = ["## Mismatches", "",
         "`%s` -> `packed_mis.json`, taken on the kernels and library of commit %s.  1 Gi symbols; call: ms per call from the device's stream events around %d back-to-back calls, %d repetitions after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches per side after a warm-up.  median [min-max].  outside: the medians differ by more than the larger of the two spreads.  The rand2 planes (128 MiB) are of Infinity-Cache size: possibly flattered.  An 8 Gi row was not taken." % (
             res.get("command"), res.get("commit"), res["batch"], res["reps"], res.get("trace_reps", 0)), "",
         "(1) The price of the counter: `psearch_mis` with k against `psearch` of the same pattern cut from the text (BITS = 1 for k = 0, 1; 2 for k = 3; 3 for k = 7).  Recorded as measured; nothing is required of it.", "",
         "| text | m | k | occurrences | psearch, ms | psearch_mis, ms | mis / exact | outside | planes_scan, us | planes_mis_scan, us | mis / exact | outside |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["counter"]:
        k = c.get("kernel_us")
        L.append("| %s%s | %d | %d | %d | %s | %s | %.3f | %s | %s | %s | %s | %s |" % (
            c["text"], note(c["text"]), c["m"], c["k"], c["count"], fmt(c["psearch_ms"]), fmt(c["psearch_mis_ms"]), c["ratio_of_medians"], "YES" if c["outside_spread"] else "no",
            fus(k["planes_scan"]) if k else "not measured", fus(k["planes_mis_scan"]) if k else "not measured",
            "%.3f" % k["ratio_of_medians"] if k else "", ("YES" if k["outside_spread"] else "no") if k else ""))
    L += ["", "(2) rand4, m = %d: ONE `psearch_mis` call against the `psearch_sets` calls, one per placement of k full-set positions, that give the same answer today (counting only, no union of the overlapping hit sets on the host: this flatters the alternative; for k = 2 a sample of the placements is timed and scaled).  REQUIRED for k = 1: the one call faster, outside the spread." % PLACE_M, "",
          "| k | placements (timed) | occurrences | psearch_mis, ms | all placements, ms | placements / one call | one call faster, outside the spread |", "|---|---|---|---|---|---|---|"]
    for c in res["placements"]:
        L.append("| %d%s | %d (%d) | %d | %s | %s | %.2f | %s |" % (c["k"], " (required)" if c["required"] else "", c["placements"], c["placements_timed"], c["count"],
                 fmt(c["psearch_mis_ms"]), fmt(c["psearch_sets_all_placements_ms"]), c["ratio_of_medians"], "YES" if c["one_call_faster_outside_spread"] else "**NO**"))
    req = [c for c in res["placements"] if c["required"]]
    if req:
        L += ["", "The required cell %s." % ("HOLDS" if all(c["one_call_faster_outside_spread"] for c in req) else "**FAILS**: one `psearch_mis` call is not faster than the placements outside the spread")]
    L += ["", "(3) `pfind_mis`, rand4, m = %d, k = %d, against `pfind_sets` of the same pattern with one full-set position (sparse output); recorded only:" % (FIND_M, FIND_K), "",
          "| occurrences (mis) | occurrences (one N) | pfind_sets, ms | pfind_mis, ms | mis / sets | outside |", "|---|---|---|---|---|---|"]
    for c in res["find"]:
        L.append("| %d | %d | %s | %s | %.3f | %s |" % (c["count"], c["count_one_N"], fmt(c["pfind_sets_ms"]), fmt(c["pfind_mis_ms"]), c["ratio_of_medians"], "YES" if c["outside_spread"] else "no"))
    if res.get("asm_diff"):
        L += ["", "(4) `python tools/asm_stats.py --diff` of the parent's `k_planes` assembly against this one (gfx950, cross-compiled; key `asm_diff` of the JSON file) — the existing plane kernels keep their instruction streams — and the new kernels' counts (key `asm_new`):", "", "```"] + res["asm_diff"] + [""] + res.get("asm_new", []) + ["```"]
    L += ["", "Choices that are NOT measured: `kUnroll` = 2 and 8 workgroups per CU as `planes_scan` (BITS = 3 on two planes: 7 per CU, its 67 / 69 VGPRs do not fit the 64 of eight waves per SIMD without scratch); the early leave every 8 symbols; two-value texts with large k and m > 32, where about 0.1 % of the positions are within the budget after 32 symbols and nearly every wave enters the verification (rows above for rand2 m = 64, 256 with k = 7 are what that costs on this text); a pre-filter on symbols 32-63 is not built."]
    path = os.path.join(os.path.dirname(a.out), "RESULTS.md")
    if not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", "packed", "RESULTS.md")
    text = open(path).read()
    at = text.find("\n## Mismatches")
    if at >= 0:
        end = text.find("\n## ", at + 1)
        text = text[:at] + (text[end:] if end >= 0 else "\n")
    text = text.rstrip("\n") + "\n\n" + "\n".join(L) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("rendered the Mismatches section of " + path)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "asm", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_mis.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "mis_probe"))
    ap.add_argument("--parent-asm", help="asm: the parent's k_planes assembly (hipcc -S --cuda-device-only)")
    ap.add_argument("--new-asm", help="asm: this tree's k_planes assembly")
    ap.add_argument("--commit", help="the commit the numbers are taken on (default: git rev-parse HEAD)")
    a = ap.parse_args()
    a.out, a.scratch = os.path.abspath(a.out), os.path.abspath(a.scratch)
    if a.step == "measure":
        return measure(a.out)
    if a.step == "workload":
        return workload(a.out)
    if a.step == "asm":
        return asm(a)
    if a.step == "render":
        return render(a)
    return driver(a) or render(a)


if __name__ == "__main__":
    sys.exit(main())
