#!/usr/bin/env python3
"""Starts and alignments of edit-distance occurrences, on the GPU: python tools/align_probe.py [--out profiles/packed/packed_align.json]

1 Gi symbols of rand4 (host-generated, so that occurrences can be planted), m = 20 / 64, k = 2 / 7.  Copies of the pattern
are written into the text at a fixed stride — a third exact, a third with one substitution, a third with one symbol removed
— as many as make the find return about 1 Mi END positions (a copy is an occurrence at its own end and, at a larger
distance, at the ends next to it: about 2 (k - 2/3) + 1 ends per copy).  m = 20 with k = 7 gets no copies: 1 Gi symbols of
rand4 hold several Mi occurrences of a random 20-mer within 7 edits by themselves, and the list is what the find returns.
Numbers only, nothing is required of them:
  pfind_edit            the call that produces the ends;
  palign_edit           on those ends, with ops (traceback) and with ops=False;
  the time per occurrence, and the headline "align adds x % to the find".
Method: host clock around each (synchronous) call — the align call's cost includes the list's way to the device and the
results' way back —, REPS repetitions after a warm-up, the three sides alternating in order from repetition to repetition;
median [min-max] is reported.  `render` writes the section "Edit distance: starts and alignments" of
profiles/packed/RESULTS.md from the JSON file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sets_probe import commit, compare, spread  # noqa: E402

N = 1 << 30
CELLS = ((20, 2, True), (20, 7, False), (64, 2, True), (64, 7, True))  # m, k, whether copies are planted
CAP = 16 << 20
REPS = 7
ACGT = (65, 67, 71, 84)
SECTION = "## Edit distance: starts and alignments"


def planted_text(np, base, P, k, rng):
    """base with copies of P every `stride` symbols; returns (text, copies)."""
    m = len(P)
    copies = int((1 << 20) / (2 * (k - 2 / 3) + 1))  # about that many ends around a copy lie within k
    stride = N // copies
    T = base.copy()
    at = (np.arange(copies, dtype=np.int64) * stride + 64)
    kind = np.arange(copies) % 3
    col = rng.integers(1, m - 1, copies)
    W = np.tile(P, (copies, 1))
    sub = kind == 1
    W[sub, col[sub]] = np.asarray(ACGT, dtype=np.uint8)[(np.searchsorted(ACGT, W[sub, col[sub]]) + 1) % 4]
    dele = kind == 2
    idx = np.arange(m)[None, :] + (np.arange(m)[None, :] >= col[:, None])  # column j and all after it: one to the right
    Wd = np.concatenate([P, P[-1:]])[np.minimum(idx, m)]
    W[dele] = Wd[dele]  # (the last column repeats P[m - 1]: one symbol of filler behind the shortened copy)
    T[at[:, None] + np.arange(m)[None, :]] = W
    return T, copies


def clock(fn):
    t0 = time.perf_counter()
    got = fn()
    return (time.perf_counter() - t0) * 1e3, got


def measure(out):
    import numpy as np
    import smart_amd
    rng = np.random.default_rng(0xA11)
    base = np.asarray(ACGT, dtype=np.uint8)[rng.integers(0, 4, N, dtype=np.uint8)]
    res = {"n": N, "reps": REPS, "unit": "ms per call (host clock around the synchronous call)", "cells": []}
    for m, k, plant in CELLS:
        P = np.asarray(ACGT, dtype=np.uint8)[rng.integers(0, 4, m)]
        T, copies = planted_text(np, base, P, k, rng) if plant else (base, 0)
        pt = smart_amd.PackedText.upload(T)
        del T
        ends, dist, count = smart_amd.pfind_edit(P, pt, k, cap=CAP)
        assert ends is not None and count >= max(copies, 1), (m, k, count, copies)
        sides = {"find": lambda: smart_amd.pfind_edit(P, pt, k, cap=CAP)[2],
                 "align_ops": lambda: smart_amd.palign_edit(P, pt, k, ends),
                 "align": lambda: smart_amd.palign_edit(P, pt, k, ends, ops=False)}
        t = {s: [] for s in sides}
        for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
            order = sorted(sides)
            order = order[rep % 3:] + order[:rep % 3]
            for s in (order if rep % 2 else order[::-1]):
                ms, got = clock(sides[s])
                if s == "find":
                    assert got == count
                else:
                    assert np.array_equal(got[1], dist) and (got[0] <= ends + np.uint64(1)).all(), (m, k, s)  # the find's distances
                t[s].append(ms)
        f, a, o = spread(t["find"][1:]), spread(t["align"][1:]), spread(t["align_ops"][1:])
        cell = {"m": m, "k": k, "copies": copies, "count": count, "pfind_edit_ms": f, "palign_edit_ms": a, "palign_edit_ops_ms": o,
                "ns_per_occurrence": a["median"] * 1e6 / count, "ns_per_occurrence_ops": o["median"] * 1e6 / count,
                "align_adds_percent": 100.0 * a["median"] / f["median"], "align_ops_adds_percent": 100.0 * o["median"] / f["median"],
                "ops_over_no_ops": compare(a, o)}
        res["cells"].append(cell)
        print("m=%-2d k=%d  %d occurrences  find %.3f ms  align %.3f ms (+%.0f %%, %.1f ns/occ)  align+ops %.3f ms (+%.0f %%, %.1f ns/occ)" % (
            m, k, count, f["median"], a["median"], cell["align_adds_percent"], cell["ns_per_occurrence"], o["median"],
            cell["align_ops_adds_percent"], cell["ns_per_occurrence_ops"]), flush=True)
        pt.free()
    res["command"] = "python tools/align_probe.py"
    res["commit"] = commit()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote " + out)
    return 0


def render(a):
    res = json.load(open(a.out))
    fmt = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    L = [SECTION, "",
         "`%s` -> `packed_align.json`, taken on the library of commit %s (the parent of the commit that adds the calls: the numbers were taken on its working tree).  1 Gi symbols of rand4 with planted copies of the pattern (a third exact, a third with one substitution, a third with one symbol removed), so that the find returns about 1 Mi end positions; m = 20 with k = 7 has no copies, rand4 itself holds that many occurrences, and with ops its list goes through several pieces of 2 Mi.  Every end the find returns is aligned.  ms per call by the host clock around the synchronous call, %d repetitions after a warm-up, the three sides in alternating order; median [min-max].  The align call's time includes the list's copy to the device and the results' copy back (8 bytes in, 8 out per occurrence, 24 more with ops)." % (
             res.get("command"), res.get("commit"), res["reps"]), "",
         "Headline: **align adds x % to the find** — the column `align / find`.  Recorded as measured; there is no target.", "",
         "| m | k | occurrences | pfind_edit, ms | palign_edit (no ops), ms | align / find | ns per occurrence | palign_edit (ops), ms | align+ops / find | ns per occurrence | ops / no ops | outside |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        L.append("| %d | %d | %d | %s | %s | +%.0f %% | %.1f | %s | +%.0f %% | %.1f | %.2f | %s |" % (
            c["m"], c["k"], c["count"], fmt(c["pfind_edit_ms"]), fmt(c["palign_edit_ms"]), c["align_adds_percent"], c["ns_per_occurrence"],
            fmt(c["palign_edit_ops_ms"]), c["align_ops_adds_percent"], c["ns_per_occurrence_ops"], c["ops_over_no_ops"]["ratio_of_medians"],
            "YES" if c["ops_over_no_ops"]["outside_spread"] else "no"))
    L += ["", "NOT measured: the kernel's own time (no kernel trace was taken, so how a call's time divides between the kernel and the copies is not known), 64 / 32 occurrences per workgroup against other sizes, the uncoalesced text loads, texts beyond 1 Gi symbols, a fused find-and-align kernel."]
    path = os.path.join(ROOT, "profiles", "packed", "RESULTS.md")
    text = open(path).read()
    at = text.find("\n" + SECTION)
    if at >= 0:
        end = text.find("\n## ", at + 1)
        text = text[:at] + (text[end:] if end >= 0 else "\n")
    text = text.rstrip("\n") + "\n\n" + "\n".join(L) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("rendered '%s' of %s" % (SECTION, path))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=("all", "measure", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "packed_align.json"))
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)
    if a.step == "measure":
        return measure(a.out)
    if a.step == "render":
        return render(a)
    return measure(a.out) or render(a)


if __name__ == "__main__":
    sys.exit(main())
