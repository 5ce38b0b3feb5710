#!/usr/bin/env python3
"""Starts and alignments of edit-distance occurrences on BYTE texts, on the GPU: python tools/talign_probe.py [--out profiles/tedit/talign.json]

1 GiB of rand128, of the English corpus (tiled) and of rand4, host-built so that occurrences can be planted; m = 20 / 64,
k = 2 / 7.  Copies of the pattern are written into the text at a fixed stride — a third exact, a third with one substitution,
a third with one byte removed — as many as make the find return about 1 Mi END positions (about 2 (k - 2/3) + 1 ends per
copy).  rand4 at m = 20, k = 7 gets no copies: it holds several Mi occurrences by itself.
Numbers only, nothing is required of them:
  find_edit             the call that produces the ends;
  align_edit            on those ends, with ops (traceback) and with ops=False: "align adds x % to the find";
  palign_edit           rand4 only: the same bytes packed, the same P, k and ends — the existing kernel, the nearest thing
                        already measured; the answers of the two are compared as well.
Method: host clock around each (synchronous) call — the align call's cost includes the list's way to the device and the
results' way back —, REPS repetitions after a warm-up, the sides alternating in order from repetition to repetition;
median [min-max] is reported.  `render` writes the section "Starts and alignments" of profiles/tedit/RESULTS.md from the
JSON file."""
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
CELLS = ((20, 2), (20, 7), (64, 2), (64, 7))
TEXTS = ("rand128", "english", "rand4")
CAP = 16 << 20
REPS = 7
SECTION = "## Starts and alignments"


def base_text(np, name, rng):
    """(1 GiB of the text, its sorted distinct values)."""
    if name == "english":
        from smart_amd import corpus
        unit = np.asarray(corpus.english_unit(), dtype=np.uint8)
        return np.resize(unit, N), np.unique(unit)
    sigma = int(name[4:])
    vals = np.asarray((65, 67, 71, 84), dtype=np.uint8) if sigma == 4 else np.arange(sigma, dtype=np.uint8)
    return vals[rng.integers(0, sigma, N, dtype=np.uint8)], vals


def planted_text(np, base, vals, P, k, rng):
    """base with copies of P every `stride` bytes; returns (text, copies)."""
    m = len(P)
    copies = int((1 << 20) / (2 * (k - 2 / 3) + 1))  # about that many ends around a copy lie within k
    stride = N // copies
    T = base.copy()
    at = (np.arange(copies, dtype=np.int64) * stride + 64)
    kind = np.arange(copies) % 3
    col = rng.integers(1, m - 1, copies)
    W = np.tile(P, (copies, 1))
    sub = kind == 1
    W[sub, col[sub]] = vals[(np.searchsorted(vals, W[sub, col[sub]]) + 1) % len(vals)]
    dele = kind == 2
    idx = np.arange(m)[None, :] + (np.arange(m)[None, :] >= col[:, None])  # column j and all after it: one to the right
    Wd = np.concatenate([P, P[-1:]])[np.minimum(idx, m)]
    W[dele] = Wd[dele]  # (the last column repeats P[m - 1]: one byte of filler behind the shortened copy)
    T[at[:, None] + np.arange(m)[None, :]] = W
    return T, copies


def clock(fn):
    t0 = time.perf_counter()
    got = fn()
    return (time.perf_counter() - t0) * 1e3, got


def measure(out):
    import numpy as np
    import smart_amd
    rng = np.random.default_rng(0x7A11)
    res = {"n": N, "reps": REPS, "unit": "ms per call (host clock around the synchronous call)", "cells": []}
    for name in TEXTS:
        base, vals = base_text(np, name, rng)
        for m, k in CELLS:
            plant = not (name == "rand4" and (m, k) == (20, 7))
            P = vals[rng.integers(0, len(vals), m)] if name != "english" else base[123456:123456 + m].copy()
            T, copies = planted_text(np, base, vals, P, k, rng) if plant else (base, 0)
            text = smart_amd.Text.upload(T)
            del T
            pt = smart_amd.PackedText.pack(text) if name == "rand4" else None
            ends, dist = smart_amd.find_edit(P, text, k, cap=CAP)
            count = len(ends)
            assert count >= max(copies, 1), (name, m, k, count, copies)
            sides = {"find": lambda: smart_amd.find_edit(P, text, k, cap=CAP)[0],
                     "align_ops": lambda: smart_amd.align_edit(P, text, k, ends),
                     "align": lambda: smart_amd.align_edit(P, text, k, ends, ops=False)}
            if pt is not None:
                sides["palign_ops"] = lambda: smart_amd.palign_edit(P, pt, k, ends)
                sides["palign"] = lambda: smart_amd.palign_edit(P, pt, k, ends, ops=False)
            t = {s: [] for s in sides}
            last = {}
            for rep in range(REPS + 1):  # repetition 0: warm-up, dropped
                order = sorted(sides)
                order = order[rep % len(order):] + order[:rep % len(order)]
                for s in (order if rep % 2 else order[::-1]):
                    ms, got = clock(sides[s])
                    if s == "find":
                        assert len(got) == count
                    else:
                        assert np.array_equal(got[1], dist) and (got[0] <= ends + np.uint64(1)).all(), (name, m, k, s)  # the find's distances
                        last[s] = got
                    t[s].append(ms)
            if pt is not None:  # the packed kernel on the same bytes: identical answers
                for a, b in (("align", "palign"), ("align_ops", "palign_ops")):
                    assert np.array_equal(last[a][0], last[b][0]) and (last[a][2] is None or np.array_equal(last[a][2], last[b][2])), (m, k, a)
            f, a, o = spread(t["find"][1:]), spread(t["align"][1:]), spread(t["align_ops"][1:])
            cell = {"text": name, "m": m, "k": k, "copies": copies, "count": count, "find_edit_ms": f, "align_edit_ms": a, "align_edit_ops_ms": o,
                    "ns_per_occurrence": a["median"] * 1e6 / count, "ns_per_occurrence_ops": o["median"] * 1e6 / count,
                    "align_adds_percent": 100.0 * a["median"] / f["median"], "align_ops_adds_percent": 100.0 * o["median"] / f["median"],
                    "ops_over_no_ops": compare(a, o)}
            if pt is not None:
                pa, po = spread(t["palign"][1:]), spread(t["palign_ops"][1:])
                cell.update({"palign_edit_ms": pa, "palign_edit_ops_ms": po, "align_over_palign": compare(pa, a), "align_ops_over_palign_ops": compare(po, o)})
                pt.free()
            text.free()
            res["cells"].append(cell)
            print("%-8s m=%-2d k=%d  %d occurrences  find %.3f ms  align %.3f ms (+%.0f %%, %.1f ns/occ)  align+ops %.3f ms (+%.0f %%, %.1f ns/occ)%s" % (
                name, m, k, count, f["median"], a["median"], cell["align_adds_percent"], cell["ns_per_occurrence"], o["median"],
                cell["align_ops_adds_percent"], cell["ns_per_occurrence_ops"],
                "  against palign_edit %.2f x / %.2f x" % (cell["align_over_palign"]["ratio_of_medians"], cell["align_ops_over_palign_ops"]["ratio_of_medians"]) if pt is not None else ""), flush=True)
            with open(out, "w") as fh:  # after every cell: a run that is cut short leaves what it measured
                json.dump(res, fh, indent=1)
        del base
    res["command"] = "python tools/talign_probe.py"
    res["commit"] = commit()
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote " + out)
    return 0


def render(a):
    res = json.load(open(a.out))
    fmt = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    L = [SECTION, "",
         "`%s` -> `%s`, taken on the working tree on top of commit %s.  1 GiB texts, host-built, with planted copies of the pattern (a third exact, a third with one substitution, a third with one byte removed), so that the find returns about 1 Mi end positions; rand4 at m = 20, k = 7 has no copies, it holds that many occurrences by itself, and with ops its list goes through several pieces of 2 Mi.  Every end the find returns is aligned.  ms per call by the host clock around the synchronous call, %d repetitions after a warm-up, the sides in alternating order; median [min-max].  The align call's time includes the list's copy to the device and the results' copy back (8 bytes in, 8 out per occurrence, 24 more with ops).  Recorded as measured; there is no target." % (
             res.get("command", "python tools/talign_probe.py"), os.path.basename(a.out), res.get("commit", "?"), res["reps"]), "",
         "### Against the find that produced the ends", "",
         "| text | m | k | occurrences | find_edit, ms | align_edit (no ops), ms | align / find | ns per occurrence | align_edit (ops), ms | align+ops / find | ns per occurrence | ops / no ops | outside |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        L.append("| %s | %d | %d | %d | %s | %s | +%.0f %% | %.1f | %s | +%.0f %% | %.1f | %.2f | %s |" % (
            c["text"], c["m"], c["k"], c["count"], fmt(c["find_edit_ms"]), fmt(c["align_edit_ms"]), c["align_adds_percent"], c["ns_per_occurrence"],
            fmt(c["align_edit_ops_ms"]), c["align_ops_adds_percent"], c["ns_per_occurrence_ops"], c["ops_over_no_ops"]["ratio_of_medians"],
            "YES" if c["ops_over_no_ops"]["outside_spread"] else "no"))
    packed = [c for c in res["cells"] if "palign_edit_ms" in c]
    if packed:
        L += ["", "### Against palign_edit on the same rand4 bytes, packed", "",
              "The same P, k and ends; the two calls' starts and operations were compared and are identical.", "",
              "| m | k | occurrences | palign_edit (no ops), ms | align_edit (no ops), ms | bytes / packed | outside | palign_edit (ops), ms | align_edit (ops), ms | bytes / packed | outside |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
        for c in packed:
            x, y = c["align_over_palign"], c["align_ops_over_palign_ops"]
            L.append("| %d | %d | %d | %s | %s | %.2f | %s | %s | %s | %.2f | %s |" % (
                c["m"], c["k"], c["count"], fmt(c["palign_edit_ms"]), fmt(c["align_edit_ms"]), x["ratio_of_medians"], "YES" if x["outside_spread"] else "no",
                fmt(c["palign_edit_ops_ms"]), fmt(c["align_edit_ops_ms"]), y["ratio_of_medians"], "YES" if y["outside_spread"] else "no"))
    missing = [t for t in TEXTS if not any(c["text"] == t for c in res["cells"])]
    L += ["", "NOT measured: %sthe kernel's own time (no kernel trace was taken, so how a call's time divides between the kernel and the copies is not known), the LDS copy of the table against reads from the arena, 64 / 32 occurrences per workgroup against other sizes, the uncoalesced window loads, the classes calls (the same kernels, another table), texts beyond 1 GiB, a fused find-and-align kernel." % (
        ("the texts " + ", ".join(missing) + " (the run was cut short), ") if missing else "")]
    path = os.path.join(ROOT, "profiles", "tedit", "RESULTS.md")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tedit", "talign.json"))
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)
    if a.step == "measure":
        return measure(a.out)
    if a.step == "render":
        return render(a)
    return measure(a.out) or render(a)


if __name__ == "__main__":
    sys.exit(main())
