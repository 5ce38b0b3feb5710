#!/usr/bin/env python3
"""The open-ended form of tests/test_packed_fuzz_gpu.py on a GPU box: the same draw and the same checks
(tests/packed_fuzz.py), any family, seed and stretch of indices; stops at the first mismatch with the case printed.
python tools/packed_fuzz_gpu.py [--family F|all] [--seed S] [--start I] [--cases N]
(not a test: run by hand after changes to the packed kernels.  A failure of the suite's fuzz names (family, index):
--family F --start I --cases 1 runs that case alone.)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import packed_fuzz as pf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--family", default="all", choices=pf.FAMILIES + ("all",))
ap.add_argument("--seed", type=int, default=pf.SEED)
ap.add_argument("--start", type=int, default=0)
ap.add_argument("--cases", type=int, default=200)
args = ap.parse_args()

for family in pf.FAMILIES if args.family == "all" else (args.family,):
    tally = pf.Tally()
    t0 = time.time()
    for index in range(args.start, args.start + args.cases):
        case = pf.draw(family, index, args.seed)
        try:
            pf.check(case, tally)
        except AssertionError as e:
            print("MISMATCH %s" % e)
            print("  text    %s%s" % (case.T[:200].tolist(), " ..." if len(case.T) > 200 else ""))
            print("  pattern %s" % case.pat.tolist())
            sys.exit(1)
    print("packed fuzz %s: cases %d .. %d, seed %d, %d comparisons in %.1f s: ALL EQUAL"
          % (family, args.start, args.start + args.cases - 1, args.seed, tally.comparisons, time.time() - t0))
