"""The rows that carry a pattern's end by value into a shared pass (multi.hpp: kTailRow, tail_fill, tail_at), on the CPU:
tests/coalesce_tail_check.cpp fills every row by the rule into a heap buffer of exactly the row size, builds the skip
table and the tails from the rows alone, as the prologue of hor_multi_scan does, and compares them entry by entry with
those built from the whole patterns; then it walks a rand256 text of 20 000 bytes 64 window ends at a time and compares
every pattern's count with brute force.  m = 3, 8, 17, 18, 64, 65, 66, 67 (both sides of the 65 bytes a row stores), 100
and 4096; groups of 1 to 8; patterns cut from the text, and patterns that share their last gram with one of them twice.
The program is compiled with AddressSanitizer and UBSan and runs without a preload: a read before a row's first stored
byte ends it, which its `before-row` mode shows."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("coalesce_tail") / "coalesce_tail_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "coalesce_tail_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    return str(exe)


def test_table_and_tails_from_the_rows_equal_those_from_the_patterns(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # 10 lengths x (8 groups cut from the text + 7 groups with one last gram)
    assert r.returncode == 0 and failures == 0 and cases == 10 * 15, r.stdout[-4000:] + r.stderr[-2000:]


def test_a_read_before_the_row_ends_the_program(program):
    r = subprocess.run([program, "before-row"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "in front of the row" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "multi.hpp" in r.stderr, r.stderr[-4000:]
