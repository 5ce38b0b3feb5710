#!/usr/bin/env python3
"""Where a timed region of bench.py spends its time, from a rocprofv3 kernel trace with per-dispatch timestamps:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python bench.py --steps 200 --warmup 50 > DIR/bench.json
    python tools/trace_gaps.py DIR/trace_kernel_trace.csv [DIR/bench.json]

The timed region is the last run of scan dispatches (hor_multi_scan, hor_sample_scan, hor_scan) that no other kernel interrupts.  Printed:
the dispatches of the region by kernel, the distribution of end(k) -> begin(k + 1) over its boundaries, the sum of the
durations against the span from the first begin to the last end, and — with bench.py's result line — the span between
the two events (kernel_ms x steps) against that, which is what lies before the first dispatch and after the last."""
import collections
import csv
import json
import statistics
import sys


def main():
    rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
    scan = lambda r: any(k in r["Kernel_Name"] for k in ("hor_multi_scan", "hor_sample_scan", "hor_scan"))  # noqa: E731
    last = max(i for i, r in enumerate(rows) if scan(r))
    first = last
    while first > 0 and scan(rows[first - 1]):
        first -= 1
    region = [(r["Kernel_Name"].split("(")[0].replace("void ", ""), int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"]) for r in rows[first:last + 1]]
    by = collections.Counter(k for k, _, _, _ in region)
    print("timed region: %d dispatches on queues %s: %s" % (len(region), sorted({q for *_, q in region}), dict(by)))
    for name in by:
        d = [(e - s) / 1e3 for k, s, e, _ in region if k == name]
        print("  %-40s n %3d  duration us: mean %.1f  min %.1f  median %.1f  max %.1f" % (name, len(d), statistics.mean(d), min(d), statistics.median(d), max(d)))
    order = sorted(region, key=lambda t: t[1])
    gaps = sorted((b[1] - a[2]) / 1e3 for a, b in zip(order, order[1:]))
    q = lambda f: gaps[min(len(gaps) - 1, int(f * len(gaps)))]  # noqa: E731
    if gaps:
        print("end(k) -> begin(k+1) over %d boundaries, us: min %.2f  p25 %.2f  median %.2f  p75 %.2f  max %.2f  sum %.1f"
              % (len(gaps), gaps[0], q(0.25), statistics.median(gaps), q(0.75), gaps[-1], sum(gaps)))
    else:
        print("end(k) -> begin(k+1): no boundary, the region is one dispatch")
    span = (max(e for _, _, e, _ in region) - order[0][1]) / 1e3
    total = sum(e - s for _, s, e, _ in region) / 1e3
    print("sum of durations %.1f us, first begin -> last end %.1f us (%.1f us of it with no scan kernel; negative: dispatches overlap)" % (total, span, span - total))
    if len(sys.argv) > 2:
        line = json.loads([x for x in open(sys.argv[2]) if x.startswith("{")][-1])
        events = line["roofline"]["kernel_ms"] * line["steps"] * 1e3
        print("event span %.0f us (kernel_ms %.4f x %d steps, +- %.0f from rounding): %.0f us outside first begin -> last end; %.1f us per dispatch, %.1f per 8 steps"
              % (events, line["roofline"]["kernel_ms"], line["steps"], 0.00005 * line["steps"] * 1e3, events - span, events / len(region), events / line["steps"] * 8))


if __name__ == "__main__":
    main()
