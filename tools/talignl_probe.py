#!/usr/bin/env python3
"""Starts and alignments of LONG edit-distance occurrences on byte texts, on the GPU:
python tools/talignl_probe.py [--out profiles/tedit/talignl.json]

1 GiB of rand128, of the English corpus (tiled) and of rand4, host-built so that occurrences can be planted; m = 64, 100, 150,
256, k = 7, 15, 31.  Copies of the pattern are written into the text at a fixed stride — a third exact, a third with one
substitution, a third with one byte removed — as many as make the find return about 1 Mi END positions (about
2 (k - 2/3) + 1 ends per copy).  A cell whose text holds more than CAP = 4 Mi occurrences by itself (rand4 at a large k and a short
pattern) is recorded as skipped.
Numbers only, nothing is required of them:
  find_editl            the call that produces the ends;
  align_editl           on those ends, with ops (decisions and traceback) and with ops=False: "align adds x % to the find";
  align_edit            m = 64, k = 7 only: the short call on the same ends — the existing kernel, unchanged; the answers of
                        the two are compared as well.
Method: host clock around each (synchronous) call — the align call's cost includes the list's way to the device and the
results' way back —, REPS repetitions after a warm-up, the sides alternating in order from repetition to repetition;
median [min-max] is reported.  `render` writes the section "Long patterns: starts and alignments" of
profiles/tedit/RESULTS.md from the JSON file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sets_probe import commit, compare, spread  # noqa: E402
from talign_probe import base_text, clock, planted_text  # noqa: E402

MS = (64, 100, 150, 256)
KS = (7, 15, 31)
TEXTS = ("rand128", "english", "rand4")
CAP = 4 << 20
REPS = 7
SECTION = "## Long patterns: starts and alignments"


def unpack(np, ops, words):
    """(count, 96 or 288) operations of rows of three or ten words, the unused ones 0, and the lengths"""
    rows = ops[:, :words - 1] if words == 10 else ops & np.array([2**64 - 1, 2**64 - 1, 2**56 - 1], dtype=np.uint64)
    length = ops[:, 9] if words == 10 else ops[:, 2] >> np.uint64(56)
    shifts = (2 * np.arange(32)).astype(np.uint64)
    return ((rows[:, :, None] >> shifts[None, None, :]) & np.uint64(3)).reshape(len(ops), -1).astype(np.uint8), length


def measure(out, texts, only):
    import numpy as np
    import smart_amd
    rng = np.random.default_rng(0x7A12)
    res = {"n": 1 << 30, "reps": REPS, "unit": "ms per call (host clock around the synchronous call)", "cells": []}
    for name in texts:
        base, vals = base_text(np, name, rng)
        for m in MS:
            for k in KS:
                if only and (m, k) not in only:
                    continue
                P = vals[rng.integers(0, len(vals), m)] if name != "english" else base[123456:123456 + m].copy()
                T, copies = planted_text(np, base, vals, P, k, rng)
                text = smart_amd.Text.upload(T)
                del T
                cell = {"text": name, "m": m, "k": k, "copies": copies}
                try:
                    ends, dist = smart_amd.find_editl(P, text, k, cap=CAP)
                except smart_amd.SmartGpuError as e:  # the text holds more than CAP occurrences by itself
                    cell["skipped"] = str(e)[:200]
                    res["cells"].append(cell)
                    text.free()
                    print("%-8s m=%-3d k=%-2d skipped: %s" % (name, m, k, cell["skipped"]), flush=True)
                    continue
                count = len(ends)
                assert count >= copies, (name, m, k, count, copies)
                sides = {"find": lambda: smart_amd.find_editl(P, text, k, cap=CAP)[0],
                         "align_ops": lambda: smart_amd.align_editl(P, text, k, ends),
                         "align": lambda: smart_amd.align_editl(P, text, k, ends, ops=False)}
                short = (m, k) == (64, 7)
                if short:
                    sides["short_ops"] = lambda: smart_amd.align_edit(P, text, k, ends)
                    sides["short"] = lambda: smart_amd.align_edit(P, text, k, ends, ops=False)
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
                if short:  # the short kernel on the same ends: identical answers
                    assert np.array_equal(last["align"][0], last["short"][0]) and np.array_equal(last["align_ops"][0], last["short_ops"][0]), (name, "starts")
                    a_ops, a_len = unpack(np, last["align_ops"][2], 10)
                    b_ops, b_len = unpack(np, last["short_ops"][2], 3)
                    assert np.array_equal(a_len, b_len) and np.array_equal(a_ops[:, :96], b_ops) and not a_ops[:, 96:].any(), (name, "operations")
                f, a, o = spread(t["find"][1:]), spread(t["align"][1:]), spread(t["align_ops"][1:])
                cell.update({"count": count, "find_editl_ms": f, "align_editl_ms": a, "align_editl_ops_ms": o,
                             "ns_per_occurrence": a["median"] * 1e6 / count, "ns_per_occurrence_ops": o["median"] * 1e6 / count,
                             "align_adds_percent": 100.0 * a["median"] / f["median"], "align_ops_adds_percent": 100.0 * o["median"] / f["median"],
                             "ops_over_no_ops": compare(a, o)})
                if short:
                    sa, so = spread(t["short"][1:]), spread(t["short_ops"][1:])
                    cell.update({"align_edit_ms": sa, "align_edit_ops_ms": so, "long_over_short": compare(sa, a), "long_ops_over_short_ops": compare(so, o)})
                text.free()
                res["cells"].append(cell)
                print("%-8s m=%-3d k=%-2d %d occurrences  find %.3f ms  align %.3f ms (+%.0f %%, %.1f ns/occ)  align+ops %.3f ms (+%.0f %%, %.1f ns/occ)%s" % (
                    name, m, k, count, f["median"], a["median"], cell["align_adds_percent"], cell["ns_per_occurrence"], o["median"],
                    cell["align_ops_adds_percent"], cell["ns_per_occurrence_ops"],
                    "  against align_edit %.2f x / %.2f x" % (cell["long_over_short"]["ratio_of_medians"], cell["long_ops_over_short_ops"]["ratio_of_medians"]) if short else ""), flush=True)
                with open(out, "w") as fh:  # after every cell: a run that is cut short leaves what it measured
                    json.dump(res, fh, indent=1)
        del base
    res["command"] = "python tools/talignl_probe.py"
    res["commit"] = commit()
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote " + out)
    return 0


def render(a):
    res = json.load(open(a.out))
    fmt = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    done = [c for c in res["cells"] if "skipped" not in c]
    L = [SECTION, "",
         "`%s` -> `%s`, taken on the working tree on top of commit %s.  1 GiB texts, host-built, with planted copies of the pattern (a third exact, a third with one substitution, a third with one byte removed), so that the find returns about 1 Mi end positions.  Every end the find returns is aligned.  ms per call by the host clock around the synchronous call, %d repetitions after a warm-up, the sides in alternating order; median [min-max].  The align call's time includes the list's copy to the device and the results' copy back (8 bytes in, 8 out per occurrence, 80 more with ops).  Recorded as measured; there is no target." % (
             res.get("command", "python tools/talignl_probe.py"), os.path.basename(a.out), res.get("commit", "?"), res["reps"]), "",
         "### Against the find that produced the ends", "",
         "| text | m | k | occurrences | find_editl, ms | align_editl (no ops), ms | align / find | ns per occurrence | align_editl (ops), ms | align+ops / find | ns per occurrence | ops / no ops | outside |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in done:
        L.append("| %s | %d | %d | %d | %s | %s | +%.0f %% | %.1f | %s | +%.0f %% | %.1f | %.2f | %s |" % (
            c["text"], c["m"], c["k"], c["count"], fmt(c["find_editl_ms"]), fmt(c["align_editl_ms"]), c["align_adds_percent"], c["ns_per_occurrence"],
            fmt(c["align_editl_ops_ms"]), c["align_ops_adds_percent"], c["ns_per_occurrence_ops"], c["ops_over_no_ops"]["ratio_of_medians"],
            "YES" if c["ops_over_no_ops"]["outside_spread"] else "no"))
    for c in res["cells"]:
        if "skipped" in c:
            L.append("| %s | %d | %d | skipped: %s |" % (c["text"], c["m"], c["k"], c["skipped"].replace("|", "/")))
    short = [c for c in done if "align_edit_ms" in c]
    if short:
        L += ["", "### Against align_edit (text_edit_align, unchanged) at m = 64, k = 7, on the same ends", "",
              "The two calls' starts, distances and unpacked operations were compared and are identical.", "",
              "| text | occurrences | align_edit (no ops), ms | align_editl (no ops), ms | long / short | outside | align_edit (ops), ms | align_editl (ops), ms | long / short | outside |",
              "|---|---|---|---|---|---|---|---|---|---|"]
        for c in short:
            x, y = c["long_over_short"], c["long_ops_over_short_ops"]
            L.append("| %s | %d | %s | %s | %.2f | %s | %s | %s | %.2f | %s |" % (
                c["text"], c["count"], fmt(c["align_edit_ms"]), fmt(c["align_editl_ms"]), x["ratio_of_medians"], "YES" if x["outside_spread"] else "no",
                fmt(c["align_edit_ops_ms"]), fmt(c["align_editl_ops_ms"]), y["ratio_of_medians"], "YES" if y["outside_spread"] else "no"))
    if done:
        adds = [c["align_adds_percent"] for c in done]
        L += ["", "The call without ops costs %.0f–%.0f %% of the find that produced its ends%s" % (
            min(adds), max(adds),
            ": a MULTIPLE of the find in the worst cells.  The follow-up for the no-ops form is a lane-per-occurrence bit-parallel walk (the block recurrence of `edit_block.hpp` in its distance form over m + k columns, no decisions kept); it is not built here." if max(adds) >= 200 else
            ".  A lane-per-occurrence bit-parallel walk for the no-ops form (the block recurrence of `edit_block.hpp` in its distance form, no decisions kept) would be cheaper in instructions; it is not built here.")]
    missing = [t for t in TEXTS if not any(c["text"] == t for c in res["cells"])]
    L += ["", "NOT measured: %sthe kernel's own time (no kernel trace was taken, so how a call's time divides between the kernel and the copies is not known), occupancy (5 to 8 workgroups per CU is what the LDS holds), DPP wave shifts against `ds_bpermute` for the neighbours' values, the serial traceback's latency, the classes calls (the same kernels, another table), texts beyond 1 GiB, packed texts." % (
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tedit", "talignl.json"))
    ap.add_argument("--texts", default=",".join(TEXTS), help="a subset of " + ",".join(TEXTS))
    ap.add_argument("--cells", default="", help="m:k,m:k,... (default: every cell)")
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)
    texts = [t for t in a.texts.split(",") if t in TEXTS]
    only = {tuple(int(x) for x in c.split(":")) for c in a.cells.split(",") if c}
    if a.step == "measure":
        return measure(a.out, texts, only)
    if a.step == "render":
        return render(a)
    return measure(a.out, texts, only) or render(a)


if __name__ == "__main__":
    sys.exit(main())
