#!/usr/bin/env python3
"""Three-plane packed texts (five to eight values), on the GPU: python tools/wide_probe.py [--out profiles/packed/packed_wide.json]

1 Gi symbols, m = 8 ... 256.  Numbers only: no threshold is set for any cell, what is measured is what gets written.
  (a) exact count on a three-plane text — rand4 over ACGT with one N as its last symbol — beside the two-plane planes_scan on
      the same symbols (the same text without the N): kernel and per-call time;
  (b) the same for psearch_mis at k = 1, 3 and 7, beside planes_mis_scan;
  (c) exact count on a rand8 text (smartgpu_text_generate, sigma = 8) and on the ACGNT text, beside the byte text's best of
      SO / BNDM / HOR for the same pattern on the same text (the comparison tools/packed_probe.py makes);
  (d) pack time per GiB.

The driver runs two steps, each a child process under its own `timeout`, and stops at the first that fails:
  1. `measure`   (a), (b) per call: the device's stream events around BATCH back-to-back calls, REPS repetitions after a
                 warm-up, the sides alternating inside every repetition; (c) as packed_probe; (d) wall clock, warm;
  2. `rocprofv3 --kernel-trace --stats -- ... workload`   kernel times of (a) and (b), a run of its own.
`render` writes the "Three planes" section of profiles/packed/RESULTS.md from the JSON file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sets_probe import commit, compare, rows_of, spread, timed  # noqa: E402

N = 1 << 30
MS = (8, 16, 32, 64, 256)
KS = (1, 3, 7)
BATCH, REPS, TRACE_REPS = 20, 10, 10
BYTE_ALGOS = ("so", "bndm", "hor")
SEED = 0x5EED0500


def acgnt_text():
    """1 Gi symbols: rand4 over ACGT, the last symbol an N."""
    import numpy as np
    T = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(SEED).integers(0, 4, N, dtype=np.uint8)]
    T[N - 1] = ord("N")
    return T


def pattern_of(T, m):
    return T[N // 3 + 17:N // 3 + 17 + m].copy()


def sides():
    return ["exact"] + list(KS)


def measure(out):
    import smart_amd
    from smart_amd import engine
    res = {"batch": BATCH, "reps": REPS, "symbols": N, "unit": "ms per call (device events around %d back-to-back calls)" % BATCH,
           "planes": [], "byte": [], "pack": {}}
    T = acgnt_text()
    text = smart_amd.Text.upload(T)
    pack_ms = []
    pt3 = None
    for _ in range(3):  # the first: cold; allocation + zero fill + planes3_pack + synchronisation, wall clock
        if pt3:
            pt3.free()
        t0 = time.perf_counter()
        pt3 = smart_amd.PackedText.pack(text, wide=True)
        pack_ms.append((time.perf_counter() - t0) * 1e3)
    pt2 = smart_amd.PackedText.upload(T[:N - 1])
    assert pt3.planes == 3 and pt2.planes == 2 and pt3.symbols() == [65, 67, 71, 78, 84]
    res["pack"]["ACGNT_1Gi"] = {"planes": 3, "plane_bytes": pt3.nbytes, "pack_wall_ms": pack_ms, "pack_wall_ms_per_GiB_of_bytes": min(pack_ms) / (N / 2**30),
                                "plane_read_GBps": [pt3.probe_read_gbs(20) for _ in range(3)]}
    # (a), (b): three planes beside two on the same symbols
    for m in MS:
        P = pattern_of(T, m)
        want = smart_amd.psearch(P, pt2, n=N - 1)[0]
        t = {(pl, s): [] for pl in (2, 3) for s in sides()}
        counts = {}
        for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
            order = [(pl, s) for s in sides() for pl in (2, 3)]
            for pl, s in (order if rep % 2 else order[::-1]):
                pt = pt3 if pl == 3 else pt2
                if s == "exact":
                    ms, got = timed(lambda: smart_amd.psearch(P, pt, n=N - 1)[0])
                    assert got == want, (m, pl, got, want)
                else:
                    ms, got = timed(lambda: smart_amd.psearch_mis(P, pt, s, n=N - 1)[0])
                    assert counts.setdefault(s, got) == got >= want, (m, pl, s, got)
                t[pl, s].append(ms)
        for s in sides():
            two, three = spread(t[2, s][1:]), spread(t[3, s][1:])
            cell = {"m": m, "k": 0 if s == "exact" else s, "call": "psearch" if s == "exact" else "psearch_mis", "count": want if s == "exact" else counts[s],
                    "two_planes_ms": two, "three_planes_ms": three}
            cell.update(compare(two, three))
            res["planes"].append(cell)
            print("m=%-4d %-7s two %.4f  three %.4f  x%.3f outside=%s" % (m, s, two["median"], three["median"], cell["ratio_of_medians"], cell["outside_spread"]), flush=True)
    pt2.free()
    # (c): the three-plane text beside the byte text, ACGNT and rand8
    for name in ("ACGNT_1Gi", "rand8_1Gi"):
        if name == "rand8_1Gi":
            pt3.free()
            text.free()
            text = smart_amd.Text.generate(SEED + 8, 8, N)
            pack_ms = []
            pt3 = None
            for _ in range(3):
                if pt3:
                    pt3.free()
                t0 = time.perf_counter()
                pt3 = smart_amd.PackedText.pack(text, wide=True)
                pack_ms.append((time.perf_counter() - t0) * 1e3)
            assert pt3.planes == 3 and len(pt3.symbols()) == 8
            res["pack"][name] = {"planes": 3, "plane_bytes": pt3.nbytes, "pack_wall_ms": pack_ms, "pack_wall_ms_per_GiB_of_bytes": min(pack_ms) / (N / 2**30),
                                 "plane_read_GBps": [pt3.probe_read_gbs(20) for _ in range(3)]}
        for m in MS:
            P = text.read(N // 3 + 17, m)
            pats = [P] * BATCH
            want = smart_amd.search("so", P, text)[0]
            packed, byte = [], {a: [] for a in BYTE_ALGOS}
            for rep in range(REPS + 1):
                engine.stream_mark(0, 0)
                counts, _ = smart_amd.psearch_batch(pats, pt3)
                engine.stream_mark(0, 1)
                ms = engine.stream_elapsed_ms(0)
                assert counts.tolist() == [want] * BATCH, (name, m, counts.tolist()[:3], want)
                if rep:
                    packed.append(N * BATCH / (ms * 1e-3))
                for a in BYTE_ALGOS:
                    c, _, run_ms, _ = smart_amd.search_batch(a, pats, text, each=True)
                    assert c.tolist() == [want] * BATCH, (name, a, m)
                    if rep:
                        byte[a].append(N * BATCH / (float(run_ms.sum()) * 1e-3))
            best = max(BYTE_ALGOS, key=lambda a: statistics.median(byte[a]))
            p, b = spread(packed), spread(byte[best])
            cell = {"text": name, "m": m, "count": want, "packed": p, "byte_best_algo": best, "byte_best": b, "byte_kernel": smart_amd.kernel_for(best, P),
                    "ratio_of_medians": p["median"] / b["median"],
                    "outside_spread": bool(abs(p["median"] - b["median"]) > max(p["max"] - p["min"], b["max"] - b["min"]))}
            res["byte"].append(cell)
            print("%-10s m=%-4d three planes %.3e  byte(%s) %.3e symbols/s  x%.2f outside=%s" % (
                name, m, p["median"], best, b["median"], cell["ratio_of_medians"], cell["outside_spread"]), flush=True)
    pt3.free()
    text.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def workload(plan_out):
    """What the kernel trace looks at: per m, planes_scan / planes3_scan and planes_mis_scan / planes3_scan with k in KS,
    TRACE_REPS + 1 times, alternating."""
    import smart_amd
    T = acgnt_text()
    pt3 = smart_amd.PackedText.upload(T, wide=True)
    pt2 = smart_amd.PackedText.upload(T[:N - 1])
    plan = []
    for m in MS:
        P = pattern_of(T, m)
        for rep in range(TRACE_REPS + 1):
            for s in sides():
                for pl, pt in ((2, pt2), (3, pt3)):
                    if s == "exact":
                        smart_amd.psearch(P, pt, n=N - 1)
                    else:
                        smart_amd.psearch_mis(P, pt, s, n=N - 1)
                    plan.append([m, s, pl, rep])
    with open(plan_out, "w") as f:
        json.dump(plan, f)


def driver(a):
    os.makedirs(a.scratch, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace_dir, plan = os.path.join(a.scratch, "wide_trace"), os.path.join(a.scratch, "wide_plan.json")
    kept = {}
    if os.path.exists(a.out):  # (e) is taken without a GPU and stored by hand: measure writes the file anew
        kept = {k: v for k, v in json.load(open(a.out)).items() if k in ("asm_diff_summary", "asm_new", "bench_ab")}
    steps = [
        ("measure", ["timeout", "-k", "10", "420"] + me + ["measure", "--out", a.out]),
        ("kernel trace", ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["workload", "--out", plan]),
    ]
    for name, cmd in steps:
        print("== " + name, flush=True)
        with open(os.path.join(a.scratch, "wide_" + name.replace(" ", "_") + ".log"), "w") as log:
            rc = subprocess.call(cmd, stdout=log if name != "measure" else None, stderr=subprocess.STDOUT, cwd=a.scratch)
        if rc != 0:
            print("step '%s' failed with exit status %d: stopping" % (name, rc))
            return rc
    res = json.load(open(a.out))
    scan = lambda r: any(k in r["Kernel_Name"] for k in ("planes_scan", "planes_mis_scan", "planes3_scan"))  # noqa: E731
    rows = sorted((r for r in rows_of(trace_dir, "kernel_trace.csv") if scan(r)), key=lambda r: int(r["Start_Timestamp"]))
    launches = json.load(open(plan))
    assert len(rows) == len(launches), (len(rows), len(launches))
    per = {}
    for r, (m, s, pl, rep) in zip(rows, launches):
        assert ("planes3_scan" in r["Kernel_Name"]) == (pl == 3), (r["Kernel_Name"], m, s, pl, rep)
        if rep:
            per.setdefault((m, s, pl), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for cell in res["planes"]:
        s = "exact" if cell["call"] == "psearch" else cell["k"]
        two, three = spread(per[(cell["m"], s, 2)]), spread(per[(cell["m"], s, 3)])
        cell["kernel_us"] = {"two_planes": two, "three_planes": three}
        cell["kernel_us"].update(compare(two, three))
    res.update(kept)
    res["trace_reps"] = TRACE_REPS
    res["command"] = "python tools/wide_probe.py"
    res["commit"] = a.commit or commit()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + a.out)
    return 0


def render(a):
    """The "Three planes" section of RESULTS.md, appended (or replaced where it stands)."""
    res = json.load(open(a.out))
    fmt = lambda v: "%.4f [%.4f-%.4f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fus = lambda v: "%.1f [%.1f-%.1f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    fsy = lambda v: "%.3e [%.3e-%.3e]" % (v["median"], v["min"], v["max"])  # noqa: E731
    L = ["## Three planes", "",
         "`%s` -> `packed_wide.json`, taken on the kernels and library of commit %s, one MI355X.  1 Gi symbols; call: ms per call from the device's stream events around %d back-to-back calls, %d repetitions after a warm-up, the sides alternating; kernel: us from a `rocprofv3 --kernel-trace` run of its own, %d dispatches per side after a warm-up.  median [min-max].  outside: the medians differ by more than the larger of the two spreads.  No threshold was set for any cell; the instruction count per position (6 against 3, 5 for a singleton) says about 2 x for (a)." % (
             res.get("command"), res.get("commit"), res["batch"], res["reps"], res.get("trace_reps", 0)), "",
         "(a), (b) A three-plane text — rand4 over `ACGT` with one `N` as its last symbol, `planes3_scan` — beside the two-plane text of the same symbols without the `N` (`planes_scan`, `planes_mis_scan`), the range leaving the last symbol out, the pattern cut from the text.  k = 0 is `psearch` (BITS = 0); k = 1, 3, 7 `psearch_mis` (BITS = 1, 2, 3):", "",
         "| m | k | occurrences | two planes, ms | three planes, ms | three / two | outside | two planes kernel, us | three planes kernel, us | three / two | outside |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["planes"]:
        k = c.get("kernel_us")
        L.append("| %d | %d | %d | %s | %s | %.3f | %s | %s | %s | %s | %s |" % (
            c["m"], c["k"], c["count"], fmt(c["two_planes_ms"]), fmt(c["three_planes_ms"]), c["ratio_of_medians"], "YES" if c["outside_spread"] else "no",
            fus(k["two_planes"]) if k else "not measured", fus(k["three_planes"]) if k else "not measured",
            "%.3f" % k["ratio_of_medians"] if k else "", ("YES" if k["outside_spread"] else "no") if k else ""))
    L += ["", "(c) Exact count on three planes (`psearch_batch`, %d launches) beside the byte text's best of SO / BNDM / HOR for the same pattern on the same text, symbols per second (the comparison of `tools/packed_probe.py`):" % res["batch"], "",
          "| text | m | occurrences | three planes, symbols/s | byte text best | byte text, symbols/s | three planes / byte | outside |", "|---|---|---|---|---|---|---|---|"]
    for c in res["byte"]:
        L.append("| %s | %d | %d | %s | %s (%s) | %s | %.2f | %s |" % (c["text"], c["m"], c["count"], fsy(c["packed"]), c["byte_best_algo"], c["byte_kernel"], fsy(c["byte_best"]),
                 c["ratio_of_medians"], "YES" if c["outside_spread"] else "no"))
    slower = [c for c in res["byte"] if c["ratio_of_medians"] < 1.0]
    L += ["", "Cells where the byte text is the faster one: %s." % (", ".join("%s m = %d (%.2f x)" % (c["text"], c["m"], c["ratio_of_medians"]) for c in slower) if slower else "none")]
    L += ["", "(d) Pack (`PackedText.pack(text, wide=True)`: allocation, zero fill, `planes3_pack`, synchronisation; wall clock, the first cold):", "",
          "| text | plane bytes | pack, ms (cold, warm, warm) | ms per GiB of text (best) | streaming read of the planes, GB/s |", "|---|---|---|---|---|"]
    for name, p in res["pack"].items():
        L.append("| %s | %d | %s | %.2f | %s |" % (name, p["plane_bytes"], ", ".join("%.2f" % x for x in p["pack_wall_ms"]), p["pack_wall_ms_per_GiB_of_bytes"],
                 ", ".join("%.0f" % x for x in p["plane_read_GBps"])))
    if res.get("asm_diff_summary"):
        L += ["", "(e) No GPU: `python tools/asm_stats.py --diff` of the parent's assembly against this one for the units `k_planes`, `k_pedit`, `k_peditl` and `k_palign` (gfx950, cross-compiled; key `asm_diff_summary` of the JSON file): %s.  The kernels of the new unit `k_planes3` (key `asm_new`):" % res["asm_diff_summary"],
              "", "```"] + res.get("asm_new", []) + ["```"]
    if res.get("bench_ab"):
        L += ["", "(f) The flagship workload is not touched by this change: %s" % res["bench_ab"]]
    L += ["", "NOT measured: the find forms, set patterns proper (every cell above is a byte pattern, so singleton sets: five instructions per position), texts of six and seven values, texts beyond 1 Gi symbols, texts with long partial matches; the occupancy choice (every `planes3_*` instantiation bounded for 128 VGPRs, 5-7 workgroups per CU) and `kUnroll` = 2 are not swept."]
    path = os.path.join(os.path.dirname(a.out), "RESULTS.md")
    if not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", "packed", "RESULTS.md")
    text = open(path).read()
    at = text.find("\n## Three planes")
    if at >= 0:
        end = text.find("\n## ", at + 1)
        text = text[:at] + (text[end:] if end >= 0 else "\n")
    text = text.rstrip("\n") + "\n\n" + "\n".join(L) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("rendered the Three planes section of " + path)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "workload", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_wide.json"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "wide_probe"))
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
