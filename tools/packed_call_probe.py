#!/usr/bin/env python3
"""Host time of the packed-text calls, two builds against each other: python tools/packed_call_probe.py --parent <library> [--new <library>]

Wall time per synchronous call (call_probe.py's manner: CALLS calls after a warm-up, patterns cut from the text) of psearch,
pfind, the six set / mismatch calls and the edit-distance calls (short and long kernels) on 64 Ki symbols of rand4, and of the
edit-distance and mismatch calls on the same symbols as a byte text, where the host dominates, at m = 16 and m = 64 — one on
each side of the pattern's staging copy; k = 1.  ROUNDS rounds per library, alternating, every round a process of its own under
its own `timeout`; stops at the first that fails.  A cell passes when the new library's median lies inside the parent's
min-max or below it.  Prints the table of the "Host path" section of profiles/packed/RESULTS.md; --out keeps the numbers."""
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

N, MS, CALLS, WARM, ROUNDS, CAP = 1 << 16, (16, 64), 300, 20, 5, 4096


def one_round():
    """us per call of every cell, as one JSON line"""
    import smart_amd
    from sets_probe import make_text, singletons
    text, pt = make_text(4, N)
    sym = pt.symbols()
    res = {}
    for m in MS:
        pats = [text.read((1000 + 3301 * j) % (N - m), m) for j in range(CALLS)]
        sets = [singletons(p, sym) for p in pats]
        for s in sets:
            s[::4] |= 1  # every fourth position accepts code 0 as well
        calls = {"psearch": lambda j: smart_amd.psearch(pats[j], pt), "pfind": lambda j: smart_amd.pfind(pats[j], pt, cap=CAP),
                 "psearch_sets": lambda j: smart_amd.psearch_sets(sets[j], pt), "pfind_sets": lambda j: smart_amd.pfind_sets(sets[j], pt, cap=CAP),
                 "psearch_mis": lambda j: smart_amd.psearch_mis(pats[j], pt, 1), "pfind_mis": lambda j: smart_amd.pfind_mis(pats[j], pt, 1, cap=CAP),
                 "psearch_sets_mis": lambda j: smart_amd.psearch_sets_mis(sets[j], pt, 1),
                 "pfind_sets_mis": lambda j: smart_amd.pfind_sets_mis(sets[j], pt, 1, cap=CAP),
                 "psearch_edit": lambda j: smart_amd.psearch_edit(pats[j], pt, 1), "pfind_edit": lambda j: smart_amd.pfind_edit(pats[j], pt, 1, cap=CAP),
                 "psearch_editl": lambda j: smart_amd.psearch_editl(pats[j], pt, 1), "pfind_editl": lambda j: smart_amd.pfind_editl(pats[j], pt, 1, cap=CAP),
                 "search_edit": lambda j: smart_amd.search_edit(pats[j], text, 1), "find_edit": lambda j: smart_amd.find_edit(pats[j], text, 1, cap=CAP),
                 "search_mis": lambda j: smart_amd.search_mis(pats[j], text, 1), "find_mis": lambda j: smart_amd.find_mis(pats[j], text, 1, cap=CAP),
                 "search_editl": lambda j: smart_amd.search_editl(pats[j], text, 1), "find_editl": lambda j: smart_amd.find_editl(pats[j], text, 1, cap=CAP)}
        for name, call in calls.items():
            for j in range(WARM):
                call(j)
            t0 = time.perf_counter()
            for j in range(CALLS):
                call(j)
            res["%s m=%d" % (name, m)] = (time.perf_counter() - t0) / CALLS * 1e6
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--round", action="store_true", help="one round on the library SMARTGPU_LIB names (what the driver starts)")
    ap.add_argument("--parent", help="the parent commit's library (tools/build_variant.sh in a worktree of it)")
    ap.add_argument("--new", default=os.path.join(ROOT, "smart_amd", "csrc", "libsmartgpu.so"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.round:
        return one_round()
    rounds = {"parent": [], "new": []}
    for r in range(ROUNDS):
        for side in (("parent", "new") if r % 2 == 0 else ("new", "parent")):
            env = dict(os.environ, SMARTGPU_LIB=os.path.abspath(getattr(a, side)))
            p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--round"], env=env, capture_output=True, text=True)
            if p.returncode != 0:
                print("round %d on %s failed with exit status %d: stopping\n%s" % (r, side, p.returncode, p.stderr[-2000:]))
                return p.returncode
            rounds[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
    print("| call | parent min / median / max, us | new median, us | new min-max, us | inside or below |\n|---|---|---|---|---|")
    ok = True
    for cell in rounds["parent"][0]:
        old, new = [r[cell] for r in rounds["parent"]], [r[cell] for r in rounds["new"]]
        inside = statistics.median(new) <= max(old)
        ok = ok and inside
        print("| %s | %.1f / %.1f / %.1f | %.1f | %.1f-%.1f | %s |" % (cell, min(old), statistics.median(old), max(old), statistics.median(new), min(new), max(new),
                                                                   "yes" if inside else "**NO**"))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"n": N, "calls": CALLS, "warm": WARM, "rounds": rounds}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
