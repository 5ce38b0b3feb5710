#!/usr/bin/env python3
"""What one queued Plan.launch costs the host, in ns, through the native binding (smart_amd._fastcall) and through the
pure-Python ctypes launch, in one process.

    python tools/launch_cost.py [--rounds 20] [--mib 2] [--root CHECKOUT] [--out FILE]
    python tools/launch_cost.py --stub          # no GPU: the binding alone, against a stub library

84 + 84 Horspool plans of m = 32 are cut from --mib MiB of rand128, once with a sample forced on the text
(smartgpu_text_sampling(0): the launches gather for hor_sample_scan) and once with the library's default (a text this
small has none: they gather for hor_multi_scan).  A round is the loop of bench.py, `for j in range(lo, hi):
plans[j].launch(text, slot=0)`, over 83 launches between two reads of the host clock: a key never fills, so no launch
of a round makes a HIP call, and the flush (device_sync) lies outside the timed part.  Per binding: the median round in
ns per launch, and the best and the worst of --rounds.  The two sets of 84 plans take turns.

--stub compiles a few lines of C (smartgpu_plan_launch, smartgpu_last_error, smartgpu_text_length: the launch stores its
arguments and returns) into a temporary directory and runs the same rounds against it: what the binding costs without
the queue; on a host without a GPU (no /dev/kfd) its lines say so.  --root imports smart_amd from another checkout (an earlier commit, which has the ctypes launch only)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

STUB_C = r"""
#include <stdint.h>
static volatile uint64_t seen[6];
int smartgpu_plan_launch(void* p, const void* t, uint64_t off, uint64_t n, int slot, int timed)
{
    seen[0] = (uint64_t)(uintptr_t)p; seen[1] = (uint64_t)(uintptr_t)t; seen[2] = off; seen[3] = n; seen[4] = (uint64_t)slot; seen[5] = (uint64_t)timed;
    return 0;
}
const char* smartgpu_last_error(void) { return ""; }
uint64_t smartgpu_text_length(const void* t) { return t ? (2u << 20) : 0; }
"""
SEED = 0x5EED0001
ROUND = 83  # one less than the narrowest full pass (84 sampled, 84 by value at m = 32)
M = 32


def streams(P):
    """A pattern whose symbols do not repeat (plan.cpp build_blob: ordered pairs of equal symbols against 1/48 of all
    pairs): its launch is one the queue counts, not a rider."""
    counts = {}
    for b in P.tolist():
        counts[b] = counts.get(b, 0) + 1
    pairs = sum(c * (c - 1) for c in counts.values())
    return pairs * 48 <= len(P) * (len(P) - 1)


def rounds_of(launch_of, plans, text, rounds, flush):
    """ns per launch of each round; launch_of(plan) is the bound method a round calls."""
    calls = [launch_of(pl) for pl in plans]
    out = []
    for r in range(rounds + 2):  # (two rounds to warm up)
        lo = (r % 2) * (ROUND + 1)
        t0 = time.perf_counter_ns()
        for j in range(lo, lo + ROUND):
            calls[j](text, slot=0)
        t1 = time.perf_counter_ns()
        flush()
        if r >= 2:
            out.append((t1 - t0) / ROUND)
    return out


def report(label, ns):
    print("%-44s ns per launch: median %7.1f  best %7.1f  worst %7.1f  (%d rounds of %d)"
          % (label, statistics.median(ns), min(ns), max(ns), len(ns), ROUND))
    return {"what": label, "median_ns": round(statistics.median(ns), 1), "best_ns": round(min(ns), 1), "worst_ns": round(max(ns), 1), "rounds": len(ns)}


def bindings(engine):
    """[(name, plan -> callable)]: the active binding's launch and, where it is another, the ctypes one."""
    ctypes_launch = getattr(engine.Plan, "_launch_ctypes", None)
    name = engine.binding() if hasattr(engine, "binding") else "ctypes"
    both = [(name, lambda pl: pl.launch)]
    if name == "native" and ctypes_launch is not None:
        both.append(("ctypes", lambda pl: pl._launch_ctypes))
    return both


def run_stub(engine, rounds, where):
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "stub.c"), os.path.join(d, "libstub.so")
        with open(src, "w") as f:
            f.write(STUB_C)
        subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, src])
        engine.use_library(so)
        text = engine.Text(0x1000)
        plans = []
        for j in range(2 * (ROUND + 1)):
            pl = engine.Plan.__new__(engine.Plan)
            pl._L = engine.lib()
            if hasattr(engine, "_bind_plan"):
                engine._bind_plan(pl)
            pl._h = 0x2000 + 64 * j
            plans.append(pl)
        rows = [report("stub library, %s%s" % (name, where), rounds_of(of, plans, text, rounds, lambda: None)) for name, of in bindings(engine)]
        t0 = time.perf_counter_ns()
        for r in range(rounds):
            for j in range(ROUND):
                plans[j]
        rows.append({"what": "the bare loop with the list index" + where, "median_ns": round((time.perf_counter_ns() - t0) / (rounds * ROUND), 1)})
        print("%-44s ns per launch: %7.1f" % (rows[-1]["what"], rows[-1]["median_ns"]))
        for pl in plans:
            pl._h = None  # (nothing to free: the stub has no smartgpu_plan_free)
        text._h = None
        return rows


def run_gpu(engine, rounds, mib):
    rows = []
    n = mib << 20
    for sampling in (0, None):
        before = engine.text_sampling(0) if sampling == 0 else None
        text = engine.Text.generate(SEED, 128, n)
        if before is not None:
            engine.text_sampling(before)
        T = text.read(0, n)
        pats, at = [], 1000
        while len(pats) < 2 * (ROUND + 1):
            P = T[at:at + M].copy()
            if streams(P) and engine.kernel_for("hor", P) == "hor_scan":
                pats.append(P)
            at += 4001
        plans = [engine.Plan("hor", P) for P in pats]
        engine.device_sync(0)
        sampled = engine.text_has_sample(text)
        for name, of in bindings(engine):
            l0, p0 = engine.coalesce_stats(0)
            ns = rounds_of(of, plans, text, rounds, lambda: engine.device_sync(0))
            l1, p1 = engine.coalesce_stats(0)
            # every launch was queued and every round left as ONE pass, sent by the flush
            assert (l1 - l0, p1 - p0) == ((rounds + 2) * ROUND, rounds + 2), (l1 - l0, p1 - p0)
            rows.append(report("%d MiB rand128, %s, %s" % (mib, "sampled" if sampled else "no sample", name), ns))
        for pl in plans:
            pl.free()
        text.free()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--mib", type=int, default=2)
    ap.add_argument("--stub", action="store_true", help="against a stub library: needs no GPU")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), help="the checkout smart_amd is imported from")
    ap.add_argument("--out", help="write the rows as JSON")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from smart_amd import engine
    print("binding: %s (%s)" % (engine.binding() if hasattr(engine, "binding") else "ctypes (a checkout without the native one)", os.path.abspath(args.root)))
    if args.stub:
        rows = run_stub(engine, args.rounds, "" if os.path.exists("/dev/kfd") else " [a CPU box: no GPU on this host]")
    else:
        rows = run_gpu(engine, args.rounds, args.mib)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
