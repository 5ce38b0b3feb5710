#!/usr/bin/env python3
"""Sweep of the shared pass (hor_multi_scan): launches per pass x workgroups per CU x pattern length on 1 GiB of rand128.

    [SMARTGPU_LIB=smart_amd/csrc/libsmartgpu_<variant>.so] python tools/coalesce_sweep.py [--ms 16,32,256] [--groups 0,2,4,8]
                                                            [--wgs 0,4,5,6,7] [--plans 24] [--rounds 5] [--out FILE]

Per cell: --plans Horspool plans (patterns cut from the text at bench.py's seeded offsets) are launched between two HIP
events on the launch stream, --rounds times; the cell is the median round in ms per pattern, with the best and the worst.
group 0 = smartgpu_coalesce(0): every launch a hor_scan of its own; wgs 0 = the library's default (smartgpu_tune(4, 0)).
Groups above 8 go through smartgpu_coalesce_wide and groups above 32 through smartgpu_coalesce_pass (a library without the
call skips them); a group above what a pass of the length takes (engine.pass_width(m)) is clipped by the library, so
--groups 96 is the widest pass at every length.  Give --plans a multiple of every group, 96 for 8, 16, 24 and 32, 168
for the widest pass at m = 32, or the last pass of a round is a partial one.  A cell also gives the kernels a round
took (smartgpu_coalesce_stats; with groups above 32 a gathering key may be sent early) and the ms per kernel.
One line per cell, and all cells as JSON in --out.  Every count is compared with the group-0 count of the same pattern."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SEED, PATTERN_SALT = 0x5EED0001, 0x0A77E2


def splitmix64(x):
    M = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def long_sweep(args):
    """--long: per length, W + 2 LW plans a round (W = engine.pass_width(m), LW = engine.long_width(m)) under the widest
    setting, once with smartgpu_coalesce_long(-1) — ceil((W + 2 LW) / W) by-value passes — and once with
    smartgpu_coalesce_long(0): the pass of W that leaves after the mark's flush, then two long passes of LW.  The same
    plans and the same events in both cells: ms per pattern, the kernels of a round, every count against the first cell's."""
    import smart_amd
    from smart_amd import Plan, Text, engine
    if smart_amd.device_count() < 1:
        raise SystemExit("no GPU: " + engine.lib().smartgpu_last_error().decode())
    n = int(args.gib * (1 << 30))
    text = Text.generate(SEED, args.sigma, n)
    engine.probe_read_gbs(text, reps=64)  # clocks
    default_group, default_long = engine.coalesce_pass(engine.PASS_MAX), engine.coalesce_long(-1)
    cells = []
    print("library %s, default group %d, default long threshold %d" % (engine.LIB_PATH, default_group, default_long))
    for m in [int(x) for x in args.ms.split(",")]:
        W, LW = engine.pass_width(m), engine.long_width(m)
        pats, j = [], 0
        while len(pats) < W + 2 * LW:
            p = text.pattern(splitmix64(PATTERN_SALT + 4096 * j + m) % (n - m), m)
            j += 1
            if engine.kernel_for("hor", p) == "hor_scan":
                pats.append(p)
        plans = [Plan("hor", p) for p in pats]
        want = None
        for least in (-1, 0):
            engine.coalesce_long(least)
            for pl in plans:
                pl.reset()
            rounds = []
            engine.device_sync(0)
            passes0 = engine.coalesce_stats(0)[1]
            for r in range(args.rounds + 1):  # round 0 warms up
                engine.stream_mark(0, 0)
                for pl in plans:
                    pl.launch(text, slot=0)
                engine.stream_mark(0, 1)
                rounds.append(engine.stream_elapsed_ms(0) / len(plans))
            engine.device_sync(0)
            passes = (engine.coalesce_stats(0)[1] - passes0) / (args.rounds + 1)
            got = [pl.result(0)[0] for pl in plans]
            want = want or got
            ok = got == want and all(c >= args.rounds + 1 and c % (args.rounds + 1) == 0 for c in got)
            rounds = sorted(rounds[1:])
            cell = {"m": m, "long": least, "width": LW if least == 0 else W, "plans": len(plans), "ms": round(rounds[len(rounds) // 2], 5),
                    "best": round(rounds[0], 5), "worst": round(rounds[-1], 5), "passes": round(passes, 2), "count_ok": ok}
            cells.append(cell)
            print("m %-4d long %-2d width %-3d plans %-3d  %.5f ms per pattern (best %.5f worst %.5f)  %.2f passes  %s"
                  % (m, least, cell["width"], len(plans), cell["ms"], cell["best"], cell["worst"], passes, "ok" if ok else "COUNT MISMATCH"), flush=True)
        for pl in plans:
            pl.free()
    engine.coalesce_long(default_long)
    engine.coalesce_pass(default_group)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"library": engine.LIB_PATH, "cells": cells}, f, indent=1)
    if not all(c["count_ok"] for c in cells):
        raise SystemExit("COUNT MISMATCH")


def sample_sweep(args):
    """--sample: sampled passes (hor_sample_scan) against hor_multi_scan, per text size (--mib) and length (--ms), in passes
    of --widths patterns (0: the long width — a round launches the by-value width and then the long width, two passes).
    Every text is created with smartgpu_text_sampling(0); a cell is measured with smartgpu_coalesce_sample on and off over
    the same text, plans and events: ms per pattern, the kernels of a round, how many of them were sampled, every count
    against the first cell's.  A library without the calls (the parent's, through SMARTGPU_LIB) measures the `off` cells
    only.  Also the host time of Text.generate per size, which holds the sample's build where the library has one."""
    import time
    import smart_amd
    from smart_amd import Plan, Text, engine
    if smart_amd.device_count() < 1:
        raise SystemExit("no GPU: " + engine.lib().smartgpu_last_error().decode())
    has = hasattr(engine.lib(), "smartgpu_coalesce_sample")
    default_group, default_long = engine.coalesce_pass(engine.PASS_MAX), engine.coalesce_long(0)
    default_sampling = engine.text_sampling(0) if has else None
    cells = []
    print("library %s, sampled passes %s" % (engine.LIB_PATH, "yes" if has else "no"))
    for mib in [int(x) for x in args.mib.split(",")]:
        n = mib << 20
        made = []
        for _ in range(3):
            t0 = time.perf_counter()
            text = Text.generate(SEED, args.sigma, n)
            made.append((time.perf_counter() - t0) * 1e3)
            text.free()
        text = Text.generate(SEED, args.sigma, n)
        engine.probe_read_gbs(text, reps=16)  # clocks
        print("%d MiB: Text.generate %.3f ms (best of 3), sample %s" % (mib, min(made), "yes" if has and engine.text_has_sample(text) else "no"), flush=True)
        for m in [int(x) for x in args.ms.split(",")]:
            for width in [int(x) for x in args.widths.split(",")]:
                want = None
                for on in ((True, False) if has else (False,)):
                    if has:
                        engine.coalesce_sample(on)
                    W = engine.SAMPLE_WIDTH if on else engine.pass_width(m)
                    LW = engine.SAMPLE_LONG_WIDTH if on else engine.long_width(m)
                    count = W + LW if width == 0 else min(width, W)
                    engine.coalesce_pass(engine.PASS_MAX if width == 0 or count >= W else max(2, count))
                    pats, j = [], 0
                    while len(pats) < count:
                        p = text.pattern(splitmix64(PATTERN_SALT + 4096 * j + m) % (n - m), m)
                        j += 1
                        if engine.kernel_for("hor", p) == "hor_scan":
                            pats.append(p)
                    plans = [Plan("hor", p) for p in pats]
                    rounds = []
                    engine.device_sync(0)
                    passes0, sampled0 = engine.coalesce_stats(0)[1], engine.coalesce_sampled(0) if has else 0
                    for r in range(args.rounds + 1):  # round 0 warms up
                        engine.stream_mark(0, 0)
                        for pl in plans:
                            pl.launch(text, slot=0)
                        engine.stream_mark(0, 1)
                        rounds.append(engine.stream_elapsed_ms(0))
                    engine.device_sync(0)
                    passes = (engine.coalesce_stats(0)[1] - passes0) / (args.rounds + 1)
                    sampled = ((engine.coalesce_sampled(0) if has else 0) - sampled0) / (args.rounds + 1)
                    got = [pl.result(0)[0] for pl in plans]
                    for pl in plans:
                        pl.free()
                    want = want or got
                    k = min(len(got), len(want))  # (the long widths differ: the patterns both cells hold)
                    ok = got[:k] == want[:k] and all(c >= args.rounds + 1 and c % (args.rounds + 1) == 0 for c in got)
                    rounds = sorted(rounds[1:])
                    cell = {"mib": mib, "m": m, "width": width, "sampled_on": bool(on), "plans": count, "ms_round": round(rounds[len(rounds) // 2], 5),
                            "best": round(rounds[0], 5), "worst": round(rounds[-1], 5), "ms_per_pattern": round(rounds[len(rounds) // 2] / count, 6),
                            "passes": round(passes, 2), "sampled": round(sampled, 2), "count_ok": ok}
                    cells.append(cell)
                    print("%5d MiB m %-4d width %-3d sample %-3s plans %-3d  %.4f ms a round (best %.4f worst %.4f) %.5f ms per pattern  %.2f passes, %.2f sampled  %s"
                          % (mib, m, width, "on" if on else "off", count, cell["ms_round"], cell["best"], cell["worst"], cell["ms_per_pattern"], passes, sampled,
                             "ok" if ok else "COUNT MISMATCH"), flush=True)
        text.free()
    if has:
        engine.coalesce_sample(True)
        engine.text_sampling(default_sampling)
    engine.coalesce_long(default_long)
    engine.coalesce_pass(default_group)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"library": engine.LIB_PATH, "cells": cells}, f, indent=1)
    if not all(c["count_ok"] for c in cells):
        raise SystemExit("COUNT MISMATCH")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", action="store_true", help="sampled passes against hor_multi_scan per text size: see sample_sweep")
    ap.add_argument("--mib", default="1,4,16,64,256,1024", help="with --sample: text sizes in MiB")
    ap.add_argument("--widths", default="8,32,84,0", help="with --sample: patterns per pass (0: the long width)")
    ap.add_argument("--ms", default="16,32,256")
    ap.add_argument("--groups", default="0,2,4,8")
    ap.add_argument("--wgs", default="0,4,5,6,7")
    ap.add_argument("--sigma", type=int, default=128)
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--plans", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--long", action="store_true", help="long passes against by-value passes: see long_sweep")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.long:
        return long_sweep(args)
    if args.sample:
        return sample_sweep(args)
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731

    import smart_amd
    from smart_amd import Plan, Text, engine
    if smart_amd.device_count() < 1:
        raise SystemExit("no GPU: " + engine.lib().smartgpu_last_error().decode())
    n = int(args.gib * (1 << 30))
    text = Text.generate(SEED, args.sigma, n)
    engine.probe_read_gbs(text, reps=64)  # clocks
    wide = hasattr(engine.lib(), "smartgpu_coalesce_wide")
    full = hasattr(engine.lib(), "smartgpu_coalesce_pass")
    set_group = engine.coalesce_pass if full else engine.coalesce_wide if wide else engine.coalesce
    default_group = set_group(8)
    cells = []
    print("library %s, default group %d" % (engine.LIB_PATH, default_group))
    for m in ints(args.ms):
        pats = []
        j = 0
        while len(pats) < args.plans:  # streaming patterns only: the others never share a pass
            p = text.pattern(splitmix64(PATTERN_SALT + 4096 * j + m) % (n - m), m)
            j += 1
            if engine.kernel_for("hor", p) == "hor_scan":
                pats.append(p)
        plans = [Plan("hor", p) for p in pats]
        want = None
        for group in ints(args.groups):
            for wgs in ints(args.wgs):
                if group == 0 and wgs != 0:
                    continue  # tune key 4 is the shared pass's
                if (group > 8 and not wide) or (group > 32 and not full):
                    continue
                set_group(group)
                engine.tune(4, wgs)
                for pl in plans:
                    pl.reset()
                rounds = []
                engine.device_sync(0)
                passes0 = engine.coalesce_stats(0)[1]
                for r in range(args.rounds + 1):  # round 0 warms up
                    engine.stream_mark(0, 0)
                    for pl in plans:
                        pl.launch(text, slot=0)
                    engine.stream_mark(0, 1)
                    rounds.append(engine.stream_elapsed_ms(0) / len(plans))
                engine.device_sync(0)
                passes = (engine.coalesce_stats(0)[1] - passes0) / (args.rounds + 1)
                got = [pl.result(0)[0] for pl in plans]
                if want is None:
                    want = got
                ok = got == want and all(c >= args.rounds + 1 and c % (args.rounds + 1) == 0 for c in got)
                rounds = sorted(rounds[1:])
                cell = {"m": m, "group": group, "wgs": wgs, "ms": round(rounds[len(rounds) // 2], 5), "best": round(rounds[0], 5),
                        "worst": round(rounds[-1], 5), "passes": round(passes, 2), "count_ok": ok}
                cell["ms_per_pass"] = round(cell["ms"] * len(plans) / passes, 5)
                cells.append(cell)
                print("m %-4d group %-2d wgs %d  %.5f ms per pattern (best %.5f worst %.5f)  %.2f passes, %.4f ms each  %s"
                      % (m, group, wgs, cell["ms"], cell["best"], cell["worst"], passes, cell["ms_per_pass"], "ok" if ok else "COUNT MISMATCH"), flush=True)
        for pl in plans:
            pl.free()
    engine.tune(4, 0)
    set_group(default_group)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"library": engine.LIB_PATH, "cells": cells}, f, indent=1)
    if not all(c["count_ok"] for c in cells):
        raise SystemExit("COUNT MISMATCH")


if __name__ == "__main__":
    main()
