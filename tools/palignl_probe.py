#!/usr/bin/env python3
"""Starts and alignments of LONG edit-distance occurrences on PACKED texts, on the GPU:
python tools/palignl_probe.py [--out profiles/packed/palignl.json]

1 Gi symbols of rand4, host-built so that occurrences can be planted, uploaded as bytes and packed on the device; m = 64, 100,
150, 256, k = 7, 31.  Copies of the pattern are written into the text at a fixed stride — a third exact, a third with one
substitution, a third with one symbol removed — as many as make the find return about 1 Mi END positions.  A cell whose text
holds more than CAP = 4 Mi occurrences by itself (rand4 at k = 31 and a short pattern) is recorded as skipped.
Numbers only, nothing is required of them:
  pfind_editl           the call that produces the ends: (c) "align adds x % to the find";
  palign_editl          on those ends, with ops (decisions and traceback) and with ops=False;
  align_editl           (a) the byte-text call on the same bytes unpacked and the same ends — the existing kernel, unchanged;
                        the answers of the two are compared bit for bit;
  palign_edit           (b) m = 64, k = 7 only: the short packed call on the same ends; starts, distances and unpacked
                        operations are compared.
Method: host clock around each (synchronous) call — an align call's cost includes the list's way to the device and the
results' way back —, REPS repetitions after a warm-up, the sides alternating in order from repetition to repetition;
median [min-max] is reported.  `render` writes the section "Long patterns: starts and alignments" of
profiles/packed/RESULTS.md from the JSON file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sets_probe import commit, compare, spread  # noqa: E402
from talign_probe import base_text, clock, planted_text  # noqa: E402
from talignl_probe import unpack  # noqa: E402

MS = (64, 100, 150, 256)
KS = (7, 31)
CAP = 4 << 20
REPS = 7
SECTION = "## Long patterns: starts and alignments"
NOT_MEASURED = "Not measured: no run of `tools/palignl_probe.py` has been recorded."


def measure(out, only):
    import numpy as np
    import smart_amd
    rng = np.random.default_rng(0x7A13)
    res = {"n": 1 << 30, "reps": REPS, "unit": "ms per call (host clock around the synchronous call)", "cells": []}
    base, vals = base_text(np, "rand4", rng)
    for m in MS:
        for k in KS:
            if only and (m, k) not in only:
                continue
            P = vals[rng.integers(0, len(vals), m)]
            T, copies = planted_text(np, base, vals, P, k, rng)
            text = smart_amd.Text.upload(T)
            del T
            pt = smart_amd.PackedText.pack(text)
            cell = {"text": "rand4", "m": m, "k": k, "copies": copies}
            ends, dist, count = smart_amd.pfind_editl(P, pt, k, cap=CAP)
            if ends is None:  # the text holds more than CAP occurrences by itself
                cell["skipped"] = "%d occurrences, more than %d" % (count, CAP)
                res["cells"].append(cell)
                pt.free()
                text.free()
                print("m=%-3d k=%-2d skipped: %s" % (m, k, cell["skipped"]), flush=True)
                continue
            assert count >= copies, (m, k, count, copies)
            sides = {"find": lambda: smart_amd.pfind_editl(P, pt, k, cap=CAP)[0],
                     "palign_ops": lambda: smart_amd.palign_editl(P, pt, k, ends),
                     "palign": lambda: smart_amd.palign_editl(P, pt, k, ends, ops=False),
                     "bytes_ops": lambda: smart_amd.align_editl(P, text, k, ends),
                     "bytes": lambda: smart_amd.align_editl(P, text, k, ends, ops=False)}
            short = (m, k) == (64, 7)
            if short:
                sides["short_ops"] = lambda: smart_amd.palign_edit(P, pt, k, ends)
                sides["short"] = lambda: smart_amd.palign_edit(P, pt, k, ends, ops=False)
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
                        assert np.array_equal(got[1], dist) and (got[0] <= ends + np.uint64(1)).all(), (m, k, s)  # the find's distances
                        last[s] = got
                    t[s].append(ms)
            # the byte kernel on the same ends: identical answers, bit for bit
            assert np.array_equal(last["palign"][0], last["bytes"][0]) and all(np.array_equal(x, y) for x, y in zip(last["palign_ops"], last["bytes_ops"])), (m, k, "bytes")
            if short:  # the short kernel on the same ends: identical answers
                assert np.array_equal(last["palign"][0], last["short"][0]) and np.array_equal(last["palign_ops"][0], last["short_ops"][0]), "starts"
                a_ops, a_len = unpack(np, last["palign_ops"][2], 10)
                b_ops, b_len = unpack(np, last["short_ops"][2], 3)
                assert np.array_equal(a_len, b_len) and np.array_equal(a_ops[:, :96], b_ops) and not a_ops[:, 96:].any(), "operations"
            f, a, o = spread(t["find"][1:]), spread(t["palign"][1:]), spread(t["palign_ops"][1:])
            ba, bo = spread(t["bytes"][1:]), spread(t["bytes_ops"][1:])
            cell.update({"count": count, "pfind_editl_ms": f, "palign_editl_ms": a, "palign_editl_ops_ms": o, "align_editl_ms": ba, "align_editl_ops_ms": bo,
                         "ns_per_occurrence": a["median"] * 1e6 / count, "ns_per_occurrence_ops": o["median"] * 1e6 / count,
                         "align_adds_percent": 100.0 * a["median"] / f["median"], "align_ops_adds_percent": 100.0 * o["median"] / f["median"],
                         "ops_over_no_ops": compare(a, o), "packed_over_bytes": compare(ba, a), "packed_ops_over_bytes_ops": compare(bo, o)})
            if short:
                sa, so = spread(t["short"][1:]), spread(t["short_ops"][1:])
                cell.update({"palign_edit_ms": sa, "palign_edit_ops_ms": so, "long_over_short": compare(sa, a), "long_ops_over_short_ops": compare(so, o)})
            pt.free()
            text.free()
            res["cells"].append(cell)
            print("m=%-3d k=%-2d %d occurrences  find %.3f ms  palign %.3f ms (+%.0f %%, %.2f x bytes)  palign+ops %.3f ms (+%.0f %%, %.2f x bytes)%s" % (
                m, k, count, f["median"], a["median"], cell["align_adds_percent"], cell["packed_over_bytes"]["ratio_of_medians"], o["median"],
                cell["align_ops_adds_percent"], cell["packed_ops_over_bytes_ops"]["ratio_of_medians"],
                "  against palign_edit %.2f x / %.2f x" % (cell["long_over_short"]["ratio_of_medians"], cell["long_ops_over_short_ops"]["ratio_of_medians"]) if short else ""), flush=True)
            with open(out, "w") as fh:  # after every cell: a run that is cut short leaves what it measured
                json.dump(res, fh, indent=1)
    res["command"] = "python tools/palignl_probe.py"
    res["commit"] = commit()
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote " + out)
    return 0


def render(a):
    res = json.load(open(a.out)) if os.path.exists(a.out) else {"cells": [], "reps": REPS}
    fmt = lambda v: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"])  # noqa: E731
    yes = lambda c: "YES" if c["outside_spread"] else "no"  # noqa: E731
    done = [c for c in res["cells"] if "skipped" not in c]
    L = [SECTION, "",
         "`smartgpu_palign_editl64` / `smartgpu_palign_sets_editl64` (`planes_editl_align`, `k_palignl.hip`): the band of `alignl_band.hpp`, one wave per listed end, fed from the bit planes.  `python tools/palignl_probe.py` takes three comparisons per cell — (a) against `align_editl` on the same bytes unpacked, (b) at m = 64, k = 7 against `palign_edit` on the same ends, (c) as a share of the `pfind_editl` that produced the ends — on 1 Gi symbols of rand4 with planted copies of the pattern (about 1 Mi ends), m = 64 / 100 / 150 / 256, k = 7 / 31, with and without ops, ms per call by the host clock around the synchronous call, %d repetitions after a warm-up, the sides in alternating order; median [min-max].  There is no target." % res["reps"], ""]
    if not done:
        L += [NOT_MEASURED]
    else:
        L += ["`%s` -> `%s`, taken on the working tree on top of commit %s." % (res.get("command", "python tools/palignl_probe.py"), os.path.basename(a.out), res.get("commit", "?")), "",
              "### (c) Against the find that produced the ends, and (a) against align_editl on the same bytes unpacked", "",
              "The packed and the byte call's starts, distances and ten words were compared and are identical.", "",
              "| m | k | occurrences | pfind_editl, ms | palign_editl (no ops), ms | align / find | align_editl (no ops), ms | packed / bytes | outside | palign_editl (ops), ms | align+ops / find | align_editl (ops), ms | packed / bytes | outside | ops / no ops |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for c in done:
            L.append("| %d | %d | %d | %s | %s | +%.0f %% | %s | %.2f | %s | %s | +%.0f %% | %s | %.2f | %s | %.2f |" % (
                c["m"], c["k"], c["count"], fmt(c["pfind_editl_ms"]), fmt(c["palign_editl_ms"]), c["align_adds_percent"], fmt(c["align_editl_ms"]),
                c["packed_over_bytes"]["ratio_of_medians"], yes(c["packed_over_bytes"]), fmt(c["palign_editl_ops_ms"]), c["align_ops_adds_percent"],
                fmt(c["align_editl_ops_ms"]), c["packed_ops_over_bytes_ops"]["ratio_of_medians"], yes(c["packed_ops_over_bytes_ops"]), c["ops_over_no_ops"]["ratio_of_medians"]))
        for c in res["cells"]:
            if "skipped" in c:
                L.append("| %d | %d | skipped: %s |" % (c["m"], c["k"], c["skipped"].replace("|", "/")))
        short = [c for c in done if "palign_edit_ms" in c]
        if short:
            L += ["", "### (b) Against palign_edit (planes_edit_align, unchanged) at m = 64, k = 7, on the same ends", "",
                  "The two calls' starts, distances and unpacked operations were compared and are identical.", "",
                  "| occurrences | palign_edit (no ops), ms | palign_editl (no ops), ms | long / short | outside | palign_edit (ops), ms | palign_editl (ops), ms | long / short | outside |",
                  "|---|---|---|---|---|---|---|---|---|"]
            for c in short:
                x, y = c["long_over_short"], c["long_ops_over_short_ops"]
                L.append("| %d | %s | %s | %.2f | %s | %s | %s | %.2f | %s |" % (
                    c["count"], fmt(c["palign_edit_ms"]), fmt(c["palign_editl_ms"]), x["ratio_of_medians"], yes(x), fmt(c["palign_edit_ops_ms"]),
                    fmt(c["palign_editl_ops_ms"]), y["ratio_of_medians"], yes(y)))
        else:
            L += ["", "(b) against `palign_edit` at m = 64, k = 7: Not measured."]
        missing = [(m, k) for m in MS for k in KS if not any((c["m"], c["k"]) == (m, k) for c in res["cells"])]
        if missing:
            L += ["", "Not measured: the cells " + ", ".join("m = %d, k = %d" % mk for mk in missing) + "."]
    L += ["", "NOT measured in any case: the kernel's own time (no kernel trace: how a call's time divides between the kernel and the copies is not known), occupancy (8 workgroups per CU is what the launcher asks for), rand2 and other one-plane texts, the sets calls (the same kernels, other masks), texts beyond 1 Gi symbols."]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "palignl.json"))
    ap.add_argument("--cells", default="", help="m:k,m:k,... (default: every cell)")
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)
    only = {tuple(int(x) for x in c.split(":")) for c in a.cells.split(",") if c}
    if a.step == "measure":
        return measure(a.out, only)
    if a.step == "render":
        return render(a)
    return measure(a.out, only) or render(a)


if __name__ == "__main__":
    sys.exit(main())
