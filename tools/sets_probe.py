#!/usr/bin/env python3
"""Set patterns on packed texts, on the GPU: python tools/sets_probe.py [--out profiles/packed/packed_sets.json]

1 Gi symbols of rand4 and of rand2, m in MS.  Three questions, numbers only (no threshold is set anywhere):
  (a) psearch_sets with SINGLETON sets against psearch of the same exact pattern (planes_sets_scan against planes_scan);
  (b) a motif with g = 1, 2, 3 full-set positions in ONE psearch_sets call against its exact expansions (4^g on four values,
      2^g on two) through psearch_batch; the counts must agree;
  (c) a pattern whose first eight positions are all two-member sets (the early leave's worst case) — as it is.

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails:
  1. `measure`   one process.  Call times: the device's stream events around BATCH back-to-back calls (each call ends in a
                 synchronisation: launch and read-back are inside, the same for both sides), REPS repetitions after a warm-up,
                 the sides alternating inside every repetition.
  2. `rocprofv3 --kernel-trace --stats -- ... workload`   kernel times of (a) and (c), a run of its own: the dispatches in
                 start order against the order the workload launched them.
`render` writes the "Set patterns" section of profiles/packed/RESULTS.md from the JSON file."""
import argparse
import csv
import glob
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = (8, 16, 32, 64, 256)
BATCH, REPS = 20, 10
TRACE_REPS = 10
TEXTS = (("rand4_1Gi", 4, 1 << 30), ("rand2_1Gi", 2, 1 << 30))
MOTIF_M, MOTIF_GAPS = 16, (5, 9, 12)  # (b): a 16-symbol pattern of the text, its positions 5 / 5, 9 / 5, 9, 12 made full sets


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def compare(a, b):
    """b over a, and whether the medians differ by more than the larger run-to-run spread."""
    return {"ratio_of_medians": b["median"] / a["median"],
            "outside_spread": bool(abs(b["median"] - a["median"]) > max(a["max"] - a["min"], b["max"] - b["min"]))}


def make_text(sigma, n):
    import smart_amd
    text = smart_amd.Text.generate(0x5EED0400 + sigma, sigma, n)
    pt = smart_amd.PackedText.pack(text)
    return text, pt


def singletons(P, symbols):
    import numpy as np
    code = {v: c for c, v in enumerate(symbols)}
    return np.asarray([1 << code[int(b)] for b in P], dtype=np.uint8)


def two_member_prefix(P, symbols):
    """(c): singletons of P, the first eight positions widened by the next code (on two values: the full set).  None when
    every position then accepts everything: the library answers that without a launch."""
    sets = singletons(P, symbols)
    k = len(symbols)
    for j in range(min(8, len(sets))):
        c = int(sets[j]).bit_length() - 1
        sets[j] |= 1 << ((c + 1) % k)
    return None if all(int(x) == (1 << k) - 1 for x in sets) else sets


def timed(fn):
    """ms per call: stream events around BATCH calls."""
    from smart_amd import engine
    engine.stream_mark(0, 0)
    for _ in range(BATCH):
        got = fn()
    engine.stream_mark(0, 1)
    return engine.stream_elapsed_ms(0) / BATCH, got


def measure(out):
    import numpy as np
    import smart_amd
    res = {"batch": BATCH, "reps": REPS, "unit": "ms per call (device events around %d back-to-back calls)" % BATCH,
           "singletons": [], "motifs": [], "worst_case": []}
    for name, sigma, n in TEXTS:
        text, pt = make_text(sigma, n)
        sym = pt.symbols()
        for m in MS:
            P = text.read(n // 3 + 17, m)
            S, W = singletons(P, sym), two_member_prefix(P, sym)
            want = smart_amd.psearch(P, pt)[0]
            exact, sets, worst = [], [], []
            wcount = None
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                order = ("exact", "sets", "worst") if rep % 2 else ("sets", "exact", "worst")
                for side in order:
                    if side == "worst" and W is None:
                        continue
                    if side == "exact":
                        ms, got = timed(lambda: smart_amd.psearch(P, pt)[0])
                        assert got == want
                        exact.append(ms)
                    elif side == "sets":
                        ms, got = timed(lambda: smart_amd.psearch_sets(S, pt)[0])
                        assert got == want, (name, m, got, want)
                        sets.append(ms)
                    else:
                        ms, wcount = timed(lambda: smart_amd.psearch_sets(W, pt)[0])
                        assert wcount >= want
                        worst.append(ms)
            e, s = spread(exact[1:]), spread(sets[1:])
            cell = {"text": name, "m": m, "count": want, "psearch_ms": e, "psearch_sets_ms": s}
            cell.update(compare(e, s))
            res["singletons"].append(cell)
            print("%-10s m=%-4d exact %.4f  singleton sets %.4f  x%.3f outside=%s" % (
                name, m, e["median"], s["median"], cell["ratio_of_medians"], cell["outside_spread"]), flush=True)
            if W is not None:
                w = spread(worst[1:])
                wc = {"text": name, "m": m, "count": wcount, "psearch_sets_ms": w, "psearch_exact_same_m_ms": e}
                wc.update(compare(e, w))
                res["worst_case"].append(wc)
                print("%-10s m=%-4d two-member prefix %.4f x%.3f (count %d)" % (name, m, w["median"], wc["ratio_of_medians"], wcount), flush=True)
        # (b) motifs with g full-set positions against their exact expansions
        P = text.read(n // 3 + 17, MOTIF_M)
        for g in (1, 2, 3):
            gaps = MOTIF_GAPS[:g]
            S = singletons(P, sym)
            S[list(gaps)] = (1 << len(sym)) - 1
            pats = []
            for fill in itertools.product(sym, repeat=g):
                Q = P.copy()
                Q[list(gaps)] = fill
                pats.append(Q)
            one, many, many_wall = [], [], []
            for rep in range(REPS + 1):
                ms, got = timed(lambda: smart_amd.psearch_sets(S, pt)[0])
                one.append(ms)
                from smart_amd import engine
                engine.stream_mark(0, 0)
                counts, wall_ms = smart_amd.psearch_batch(pats, pt)
                engine.stream_mark(0, 1)
                many.append(engine.stream_elapsed_ms(0))
                many_wall.append(wall_ms)
                assert got == int(np.sum(counts)), (name, g, got, counts.tolist())
            o, b = spread(one[1:]), spread(many[1:])
            cell = {"text": name, "m": MOTIF_M, "g": g, "expansions": len(pats), "count": got, "counts_agree": True,
                    "psearch_sets_ms": o, "psearch_batch_ms": b, "psearch_batch_wall_ms": spread(many_wall[1:]),
                    "batch_over_sets": b["median"] / o["median"]}
            res["motifs"].append(cell)
            print("%-10s motif g=%d: one psearch_sets call %.4f ms, %d expansions by psearch_batch %.4f ms: x%.2f (count %d)" % (
                name, g, o["median"], len(pats), b["median"], cell["batch_over_sets"], got), flush=True)
        pt.free()
        text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per text and m, planes_scan (exact), planes_sets_scan (singletons) and
    planes_sets_scan (two-member prefix), alternating, TRACE_REPS + 1 times; the order goes to plan_out."""
    import smart_amd
    plan = []
    for name, sigma, n in TEXTS:
        text, pt = make_text(sigma, n)
        sym = pt.symbols()
        for m in MS:
            P = text.read(n // 3 + 17, m)
            S, W = singletons(P, sym), two_member_prefix(P, sym)
            for rep in range(TRACE_REPS + 1):
                smart_amd.psearch(P, pt)
                plan.append([name, m, "exact", rep])
                smart_amd.psearch_sets(S, pt)
                plan.append([name, m, "sets", rep])
                if W is not None:
                    smart_amd.psearch_sets(W, pt)
                    plan.append([name, m, "worst", rep])
        pt.free()
        text.free()
    with open(plan_out, "w") as f:
        json.dump(plan, f)


def rows_of(d, suffix):
    for f in sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                yield r


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "sets_trace"), os.path.join(a.scratch, "sets_plan.json")
    steps = [
        ("measure", ["timeout", "-k", "10", "420"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "sets_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    rows = [r for r in rows_of(trace_dir, "kernel_trace.csv") if "planes_scan" in r["Kernel_Name"] or "planes_sets_scan" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    for r, (name, m, kind, rep) in zip(rows, launches):
        assert ("planes_sets_scan" in r["Kernel_Name"]) == (kind != "exact"), (r["Kernel_Name"], name, m, kind, rep)
        if rep:
            per.setdefault((name, m), {"exact": [], "sets": [], "worst": []})[kind].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for key, kind in (("singletons", "sets"), ("worst_case", "worst")):
        for cell in res[key]:
            k = per[(cell["text"], cell["m"])]
            e, s = spread(k["exact"]), spread(k[kind])
            cell["kernel_us"] = {"planes_scan": e, "planes_sets_scan": s}
            cell["kernel_us"].update(compare(e, s))
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/sets_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def render(a):
    """The "Set patterns" section of RESULTS.md (before "## Positions", which tools/packed_probe.py keeps last)."""
    res = json.load(open(a.out))
    fmt = lambda v: "%.4f [%.4f-%.4f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.1f [%.1f-%.1f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    note = lambda t: " (possibly flattered)" if t.startswith("rand2") else ""  # noqa: E731
    L = ["## Set patterns", "",
         "`%s` -> `packed_sets.json`, taken on the kernels and library of commit %s.  1 Gi symbols; call: ms per call from the device's stream events around %d back-to-back calls (launch, read-back and synchronisation inside, the same on both sides), %d repetitions after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches per side after a warm-up.  median [min-max].  outside: the medians differ by more than the larger of the two spreads.  The rand2 planes (128 MiB) are of Infinity-Cache size and read again and again: possibly flattered, as above." % (
             res.get("command"), res.get("commit"), res["batch"], res["reps"], res.get("trace_reps", 0)), "",
         "(a) Singleton sets against the exact pattern — `psearch_sets` / `planes_sets_scan` against `psearch` / `planes_scan` (unchanged instruction stream, so the parent's kernel):", "",
         "| text | m | occurrences | psearch, ms | psearch_sets, ms | sets / exact | outside | planes_scan, us | planes_sets_scan, us | sets / exact | outside |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["singletons"]:
        k = c.get("kernel_us")
        L.append("| %s%s | %d | %d | %s | %s | %.3f | %s | %s | %s | %s | %s |" % (
            c["text"], note(c["text"]), c["m"], c["count"], fmt(c["psearch_ms"]), fmt(c["psearch_sets_ms"]), c["ratio_of_medians"], "YES" if c["outside_spread"] else "no",
            fus(k["planes_scan"]) if k else "not measured", fus(k["planes_sets_scan"]) if k else "not measured",
            "%.3f" % k["ratio_of_medians"] if k else "", ("YES" if k["outside_spread"] else "no") if k else ""))
    ks = [c["kernel_us"] for c in res["singletons"] if c.get("kernel_us")]
    if ks:
        out = [c for c in res["singletons"] if c.get("kernel_us") and c["kernel_us"]["outside_spread"]]
        L += ["", "Kernel ratio sets / exact over the cells: %.3f-%.3f; outside the run-to-run spread in %s." % (
            min(k["ratio_of_medians"] for k in ks), max(k["ratio_of_medians"] for k in ks),
            ", ".join("%s m = %d (%.3f)" % (c["text"], c["m"], c["kernel_us"]["ratio_of_medians"]) for c in out) if out else "no cell")]
        if out:
            L.append("Parity with the exact matcher was the expectation from the instruction count per position; in the cells named it does NOT hold.  What the sets kernels add is the scalar switch over the position's set for every position and chunk, and a larger loop body; this is recorded as measured, not tuned.")
    L += ["", "(b) A %d-symbol pattern of the text with g positions made full sets, ONE `psearch_sets` call, against its exact expansions through `psearch_batch` (one launch and one pass over the planes each; device events around the batch); the counts agree in every cell:" % MOTIF_M, "",
          "| text | g | expansions | occurrences | psearch_sets, ms | psearch_batch, ms | batch / sets |", "|---|---|---|---|---|---|---|"]
    for c in res["motifs"]:
        L.append("| %s%s | %d | %d | %d | %s | %s | %.2f |" % (c["text"], note(c["text"]), c["g"], c["expansions"], c["count"], fmt(c["psearch_sets_ms"]), fmt(c["psearch_batch_ms"]), c["batch_over_sets"]))
    L += ["", "(c) The first eight positions all two-member sets (on two values: full sets, which cost no instruction but kill nothing; m = 8 is then all full sets and answered without a launch: no row), the rest singletons — the early leave's worst case — against the exact pattern of the same length, recorded as it is:", "",
          "| text | m | occurrences | psearch_sets, ms | sets / exact (call) | planes_sets_scan, us | planes_scan (exact), us | sets / exact (kernel) |", "|---|---|---|---|---|---|---|---|"]
    for c in res["worst_case"]:
        k = c.get("kernel_us")
        L.append("| %s%s | %d | %d | %s | %.3f | %s | %s | %s |" % (c["text"], note(c["text"]), c["m"], c["count"], fmt(c["psearch_sets_ms"]), c["ratio_of_medians"],
                 fus(k["planes_sets_scan"]) if k else "not measured", fus(k["planes_scan"]) if k else "not measured", "%.3f" % k["ratio_of_medians"] if k else ""))
    if res.get("asm_diff"):
        L += ["", "`python tools/asm_stats.py --diff` of the parent's `k_planes` assembly against this one (gfx950, cross-compiled; key `asm_diff` of the JSON file) — the exact kernels keep their instruction streams:", "", "```"] + res["asm_diff"] + ["```"]
    L += ["", "Not measured: `pfind_sets`' speed, texts with long partial matches, texts beyond 1 Gi symbols (the planes of 1 Gi rand4 are 256 MiB, the Infinity Cache's size: these rows carry the caveat of the counting table too)."]
    path = os.path.join(os.path.dirname(a.out), "RESULTS.md")
    if not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", "packed", "RESULTS.md")
    text = open(path).read()
    at = text.find("\n## Set patterns")
    if at >= 0:
        end = text.find("\n## ", at + 1)
        text = text[:at] + (text[end:] if end >= 0 else "\n")
    pos = text.find("\n## Positions")
    section = "\n" + "\n".join(L) + "\n"
    text = text[:pos] + section + text[pos:] if pos >= 0 else text.rstrip("\n") + "\n" + section
    with open(path, "w") as f:
        f.write(text)
    print("rendered the Set patterns section of " + path)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_sets.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "sets_probe"))
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
