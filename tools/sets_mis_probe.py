#!/usr/bin/env python3
"""Set patterns with mismatches on packed texts, on the GPU: python tools/sets_mis_probe.py [--out profiles/packed/packed_sets_mis.json]

1 Gi symbols of rand4, m in MS.  Numbers only; no threshold is fixed beforehand:
  (1) the price of the switch: psearch_sets_mis with SINGLETON sets against psearch_mis of the same pattern, k = 0, 1, 3, 7;
  (2) the price of the counter: psearch_sets_mis with k = 0 against psearch_sets of the same set pattern (every fourth
      position widened to two members);
  (3) m = 16, k = 1, a pattern with g = 1, 2, 3 two-member positions: ONE pfind_sets_mis call against the 2^g pfind_mis calls
      over its exact expansions — the only correct route without these calls; their device calls alone are timed, the union
      on the host is not (a lower bound for that side).  The positions and distances of the one call must equal the union
      with the minimum distance: asserted.

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails:
  1. `measure`   call times: the device's stream events around BATCH back-to-back calls, REPS repetitions after a warm-up, the
                 sides alternating inside every repetition;
  2. `rocprofv3 --kernel-trace --stats -- ... workload`   kernel times of (1) and (2), a run of its own.
`asm --parent-asm A.s --new-asm B.s` needs no GPU: it stores `tools/asm_stats.py --diff` of the parent's `k_planes` assembly
against this one, and the new kernels' counts, in the JSON file (keys `asm_diff`, `asm_new`); the driver keeps both keys.
`render` writes the "Set patterns with mismatches" section of profiles/packed/RESULTS.md from the JSON file (the method is
tools/sets_probe.py's)."""
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
TEXT = ("rand4_1Gi", 4, 1 << 30)
EXP_M, EXP_K, EXP_GS = 16, 1, (1, 2, 3)
SECTION = "## Set patterns with mismatches"


def widened(P, sym, places):
    """singletons of P with the positions `places` widened by the next code: two-member sets"""
    S = singletons(P, sym)
    for j in places:
        c = int(S[j]).bit_length() - 1
        S[j] |= 1 << ((c + 1) % len(sym))
    return S


def expansions(S, sym):
    """the exact patterns (bytes) a set pattern stands for"""
    import numpy as np
    members = [[sym[c] for c in range(len(sym)) if int(s) >> c & 1] for s in S]
    return [np.asarray(p, dtype=np.uint8) for p in itertools.product(*members)]


def measure(out):
    import numpy as np
    import smart_amd
    res = {"batch": BATCH, "reps": REPS, "unit": "ms per call (device events around %d back-to-back calls)" % BATCH,
           "switch": [], "counter": [], "expansions": []}
    name, sigma, n = TEXT
    text, pt = make_text(sigma, n)
    sym = pt.symbols()
    for m in MS:
        P = text.read(n // 3 + 17, m)
        S = singletons(P, sym)
        # (1) singleton sets against the mismatch matcher
        for k in KS:
            a, b = [], []
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                for side in (("mis", "sets_mis") if rep % 2 else ("sets_mis", "mis")):
                    if side == "mis":
                        ms, want = timed(lambda: smart_amd.psearch_mis(P, pt, k)[0])
                        a.append(ms)
                    else:
                        ms, got = timed(lambda: smart_amd.psearch_sets_mis(S, pt, k)[0])
                        b.append(ms)
            assert got == want, (m, k, got, want)
            ea, eb = spread(a[1:]), spread(b[1:])
            cell = {"text": name, "m": m, "k": k, "count": got, "psearch_mis_ms": ea, "psearch_sets_mis_ms": eb}
            cell.update(compare(ea, eb))
            res["switch"].append(cell)
            print("(1) m=%-4d k=%d mis %.4f  sets_mis %.4f  x%.3f outside=%s (count %d)" % (
                m, k, ea["median"], eb["median"], cell["ratio_of_medians"], cell["outside_spread"], got), flush=True)
        # (2) k = 0 against the set matcher
        W = widened(P, sym, range(0, m, 4))
        a, b = [], []
        for rep in range(REPS + 1):
            for side in (("sets", "sets_mis") if rep % 2 else ("sets_mis", "sets")):
                if side == "sets":
                    ms, want = timed(lambda: smart_amd.psearch_sets(W, pt)[0])
                    a.append(ms)
                else:
                    ms, got = timed(lambda: smart_amd.psearch_sets_mis(W, pt, 0)[0])
                    b.append(ms)
        assert got == want, (m, got, want)
        ea, eb = spread(a[1:]), spread(b[1:])
        cell = {"text": name, "m": m, "count": got, "psearch_sets_ms": ea, "psearch_sets_mis_k0_ms": eb}
        cell.update(compare(ea, eb))
        res["counter"].append(cell)
        print("(2) m=%-4d sets %.4f  sets_mis k=0 %.4f  x%.3f outside=%s (count %d)" % (
            m, ea["median"], eb["median"], cell["ratio_of_medians"], cell["outside_spread"], got), flush=True)
    # (3) one call against the expansions
    P = text.read(n // 3 + 17, EXP_M)
    for g in EXP_GS:
        W = widened(P, sym, [3, 8, 13][:g])
        exps = expansions(W, sym)
        assert len(exps) == 2 ** g
        pos, dist, cnt = smart_amd.pfind_sets_mis(W, pt, EXP_K)
        best = {}
        for E in exps:
            ep, ed, _ = smart_amd.pfind_mis(E, pt, EXP_K)
            for p, d in zip(ep.tolist(), ed.tolist()):
                best[p] = min(d, best.get(p, 99))
        assert cnt == len(best) and pos.tolist() == sorted(best) and dist.tolist() == [best[p] for p in sorted(best)], (g, cnt, len(best))
        one, many = [], []
        for rep in range(REPS + 1):
            for side in (("one", "many") if rep % 2 else ("many", "one")):
                if side == "one":
                    ms, _ = timed(lambda: smart_amd.pfind_sets_mis(W, pt, EXP_K)[2])
                    one.append(ms)
                else:
                    tot = 0.0
                    for E in exps:
                        ms, _ = timed(lambda: smart_amd.pfind_mis(E, pt, EXP_K)[2])
                        tot += ms
                    many.append(tot)
        o, a = spread(one[1:]), spread(many[1:])
        cell = {"text": name, "m": EXP_M, "k": EXP_K, "g": g, "expansions": len(exps), "count": cnt, "equal_to_union_with_min_distance": True,
                "pfind_sets_mis_ms": o, "pfind_mis_all_expansions_ms": a}
        cell.update(compare(o, a))
        cell["one_call_faster_outside_spread"] = bool(cell["outside_spread"] and a["median"] > o["median"])
        res["expansions"].append(cell)
        print("(3) g=%d: one pfind_sets_mis call %.4f ms, %d pfind_mis calls %.4f ms: x%.2f outside=%s (count %d)" % (
            g, o["median"], len(exps), a["median"], cell["ratio_of_medians"], cell["outside_spread"], cnt), flush=True)
    pt.free()
    text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per m, planes_mis_scan and planes_sets_mis_scan with k in KS, planes_sets_scan and
    planes_sets_mis_scan (k = 0) on the widened pattern, TRACE_REPS + 1 times."""
    import smart_amd
    plan = []
    name, sigma, n = TEXT
    text, pt = make_text(sigma, n)
    sym = pt.symbols()
    for m in MS:
        P = text.read(n // 3 + 17, m)
        S, W = singletons(P, sym), widened(P, sym, range(0, m, 4))
        for rep in range(TRACE_REPS + 1):
            for k in KS:
                smart_amd.psearch_mis(P, pt, k)
                plan.append([m, "mis", k, rep])
                smart_amd.psearch_sets_mis(S, pt, k)
                plan.append([m, "sets_mis", k, rep])
            smart_amd.psearch_sets(W, pt)
            plan.append([m, "sets", "w", rep])
            smart_amd.psearch_sets_mis(W, pt, 0)
            plan.append([m, "sets_mis", "w", rep])
    pt.free()
    text.free()
    with open(plan_out, "w") as f:
        json.dump(plan, f)


KERNEL_OF = {"mis": "planes_mis_scan", "sets_mis": "planes_sets_mis_scan", "sets": "planes_sets_scan"}


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "sets_mis_trace"), os.path.join(a.scratch, "sets_mis_plan.json")
    kept = {}
    if os.path.exists(a.out):  # part (4) is taken without a GPU (`asm`): measure writes the file anew
        kept = {k: v for k, v in json.load(open(a.out)).items() if k in ("asm_diff", "asm_new")}
    steps = [
        ("measure", ["timeout", "-k", "10", "300"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "sets_mis_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if any(k in r["Kernel_Name"] for k in KERNEL_OF.values())]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    for r, (m, kind, k, rep) in zip(rows, launches):
        assert KERNEL_OF[kind] in r["Kernel_Name"], (r["Kernel_Name"], m, kind, k, rep)
        if rep:
            per.setdefault((m, kind, k), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for cell in res["switch"]:
        e, s = spread(per[(cell["m"], "mis", cell["k"])]), spread(per[(cell["m"], "sets_mis", cell["k"])])
        cell["kernel_us"] = {"planes_mis_scan": e, "planes_sets_mis_scan": s}
        cell["kernel_us"].update(compare(e, s))
    for cell in res["counter"]:
        e, s = spread(per[(cell["m"], "sets", "w")]), spread(per[(cell["m"], "sets_mis", "w")])
        cell["kernel_us"] = {"planes_sets_scan": e, "planes_sets_mis_scan": s}
        cell["kernel_us"].update(compare(e, s))
    res.update(kept)
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/sets_mis_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def asm(a):
    """Part (4), on the build machine: the assembly diff and the new kernels' counts into the JSON file."""
    stats = [sys.executable, os.path.join(ROOT, "tools", "asm_stats.py")]
    diff = subprocess.check_output(stats + ["--diff", a.parent_asm, a.new_asm], text=True).splitlines()
    new = [l[:118] for l in subprocess.check_output(stats + [a.new_asm], text=True).splitlines() if "planes_sets_mis_" in l]
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res["asm_diff"], res["asm_new"] = [l[:118] for l in diff], new
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("stored asm_diff (%d lines) and asm_new (%d kernels) in %s" % (len(diff), len(new), a.out))
    return 0


def render(a):
    """The section of RESULTS.md, appended (or replaced where it stands)."""
    res = json.load(open(a.out))
    fmt = lambda v: "%.4f [%.4f-%.4f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.1f [%.1f-%.1f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    yes = lambda b: "YES" if b else "no"  # noqa: E731

    def kernel_cols(c, a_, b_):
        k = c.get("kernel_us")
        return (fus(k[a_]), fus(k[b_]), "%.3f" % k["ratio_of_medians"], yes(k["outside_spread"])) if k else ("not measured", "not measured", "", "")

    L = [SECTION, "",
         "`%s` -> `packed_sets_mis.json`, taken on the kernels and library of %s.  1 Gi symbols of rand4; call: ms per call from the device's stream events around %d back-to-back calls, %d repetitions after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches per side after a warm-up.  median [min-max].  outside: the medians differ by more than the larger of the two spreads.  No threshold was fixed beforehand." % (
             res.get("command"), ("commit " + res["commit"]) if res.get("commit") else "this change", res["batch"], res["reps"], res.get("trace_reps", 0)), "",
         "(1) The price of the switch: `psearch_sets_mis` with singleton sets against `psearch_mis` of the same pattern cut from the text.", "",
         "| m | k | occurrences | psearch_mis, ms | psearch_sets_mis, ms | sets_mis / mis | outside | planes_mis_scan, us | planes_sets_mis_scan, us | sets_mis / mis | outside |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["switch"]:
        L.append("| %d | %d | %d | %s | %s | %.3f | %s | %s | %s | %s | %s |" % ((c["m"], c["k"], c["count"], fmt(c["psearch_mis_ms"]), fmt(c["psearch_sets_mis_ms"]),
                 c["ratio_of_medians"], yes(c["outside_spread"])) + kernel_cols(c, "planes_mis_scan", "planes_sets_mis_scan")))
    L += ["", "(2) The price of the counter: `psearch_sets_mis` with k = 0 against `psearch_sets` of the same set pattern (singletons cut from the text, every fourth position widened to two members).", "",
          "| m | occurrences | psearch_sets, ms | psearch_sets_mis k = 0, ms | sets_mis / sets | outside | planes_sets_scan, us | planes_sets_mis_scan, us | sets_mis / sets | outside |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["counter"]:
        L.append("| %d | %d | %s | %s | %.3f | %s | %s | %s | %s | %s |" % ((c["m"], c["count"], fmt(c["psearch_sets_ms"]), fmt(c["psearch_sets_mis_k0_ms"]),
                 c["ratio_of_medians"], yes(c["outside_spread"])) + kernel_cols(c, "planes_sets_scan", "planes_sets_mis_scan")))
    L += ["", "(3) m = %d, k = %d, g two-member positions: ONE `pfind_sets_mis` call against the 2^g `pfind_mis` calls over the pattern's exact expansions (their calls only: the union with the minimum distance on the host is not timed, a lower bound for that side).  The one call's positions and distances equal that union: asserted by the probe." % (EXP_M, EXP_K), "",
          "| g | expansions | occurrences | pfind_sets_mis, ms | all expansions, ms | expansions / one call | one call faster, outside the spread |", "|---|---|---|---|---|---|---|"]
    for c in res["expansions"]:
        L.append("| %d | %d | %d | %s | %s | %.2f | %s |" % (c["g"], c["expansions"], c["count"], fmt(c["pfind_sets_mis_ms"]), fmt(c["pfind_mis_all_expansions_ms"]),
                 c["ratio_of_medians"], "YES" if c["one_call_faster_outside_spread"] else "**NO**"))
    if res.get("asm_diff"):
        L += ["", "(4) `python tools/asm_stats.py --diff` of the parent's `k_planes` assembly against this one (gfx950, cross-compiled; key `asm_diff` of the JSON file) — `planes_scan`, `planes_find`, `planes_sets_*` and `planes_mis_*` keep their instruction streams — and the new kernels' counts (key `asm_new`):", "", "```"] + res["asm_diff"] + [""] + res.get("asm_new", []) + ["```"]
    L += ["", "Choices that are NOT measured: the occupancy (taken over from `planes_mis_*`: 8 workgroups per CU, 7 for BITS = 3 on two planes), `kUnroll` = 2, the early leave every 8 positions, two-value texts, patterns of wide sets with a large k (few windows leave early)."]
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
    print("rendered the section of " + path)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "asm", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_sets_mis.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "sets_mis_probe"))
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
