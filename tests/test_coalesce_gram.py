"""The skip table that the patterns of a shared pass use (multi.hpp: slot function, shift rule, cap), on the CPU:
tests/coalesce_gram_check.cpp builds the table serially with the functions hor_multi_scan uses, walks a text 64 window
ends at a time as a lane walks its segment and compares every pattern's count with brute force — rand256, rand128 and
rand8 texts of 20 000 bytes, groups of 1 to 8, m = 8, 9, 17, 18, 66 and 100 (above the shift cap of 64 + 1), patterns
that share their last gram, two identical patterns, and a pattern planted with its end at every residue mod 64.
The program is compiled with AddressSanitizer and UBSan: a read before the text or past the table ends it."""
import os
import re
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_shared_gram_walk_counts_like_brute_force(tmp_path):
    exe = tmp_path / "coalesce_gram_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "coalesce_gram_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # 3 texts x 6 lengths x (8 groups x 2 + 7 groups x 2)
    assert r.returncode == 0 and failures == 0 and cases == 3 * 6 * 30, r.stdout[-4000:] + r.stderr[-2000:]
