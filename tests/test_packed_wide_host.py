"""What the calls on a three-plane packed text decide on the host (smart_amd/csrc/planes3_host.hpp), on the CPU:
tests/packed_wide_check.cpp checks every bit of the eight membership planes that encode_sets8 and the byte-pattern encoder
(pattern_sets8, encode_pattern8) write against the definition in planes3.hpp — text alphabets of 5, 6 and 8 values, m = 1,
31, 32, 33, 64, 65 and SMARTGPU_XSIZE, sets with empty, full and singleton positions, empty positions kept and filled,
patterns with no, one and several foreign bytes, a bit at or above nvalues, zero bits from m up to the planes' end — with
the empty and foreign counts, the full flag and the first position of a bad set.
The program is compiled with AddressSanitizer and UBSan: a write past a plane ends it."""
import os
import re
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_wide_encoders_on_the_host(tmp_path):
    exe = tmp_path / "packed_wide_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "packed_wide_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # encode_sets8: 3 alphabets x 7 lengths x 2 rules for empty positions x 3 kinds of sets, and a bad set where a bit can be
    # one (5 and 6 values) x 7 x 2; the byte pattern: 3 x 7 x 3 kinds of pattern x 2 rules for foreign positions
    assert r.returncode == 0 and failures == 0 and cases == 3 * 7 * 2 * 3 + 2 * 7 * 2 + 3 * 7 * 3 * 2, r.stdout[-4000:] + r.stderr[-2000:]
