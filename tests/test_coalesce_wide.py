"""A shared pass of up to 32 patterns without a device.

tests/coalesce_wide_check.cpp builds the skip table of multi.hpp with a class bit per pattern (pattern g sets bit g & 7)
from rows filled by tail_fill, walks 20 000-byte rand8, rand128 and rand256 texts as hor_multi_scan does — tag test, the
patterns c, c + 8, c + 16, c + 24 of every class bit, whole compares — and compares every count with brute force:
m = 3, 8, 17, 18, 33, 66, 100, groups of 1 to 32, and groups with two patterns of one class that share their last gram,
one whole pattern twice in a class and one last gram in two classes; every shift lies in [1, gram_default(m)].  The
program is compiled with AddressSanitizer and UBSan and runs as a program, without a preload.

The setting: smartgpu_coalesce_wide takes 0 and 2..32, smartgpu_coalesce stays its narrow view (0, 2..8, a wider
previous value reported as 8)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

from smart_amd import engine

HIPCC = "/opt/rocm/bin/hipcc"
MULTI_MAX = 32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("coalesce_wide") / "coalesce_wide_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "coalesce_wide_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    return str(exe)


def test_walk_with_class_bits_counts_like_brute_force(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # 3 texts x 7 lengths x (32 groups cut from the text + 23 groups of ten or more with class mates)
    assert r.returncode == 0 and failures == 0 and cases == 3 * 7 * (32 + 23), r.stdout[-4000:] + r.stderr[-2000:]


def test_the_two_calls_set_one_number():
    L = engine.lib()
    wide, narrow = L.smartgpu_coalesce_wide, L.smartgpu_coalesce
    default = wide(0)
    try:
        assert default == 0 or 2 <= default <= MULTI_MAX
        prev = 0
        for g in (2, 3, 8, 9, 15, 16, 17, 31, 32, 0, 32):
            assert wide(g) == prev
            prev = g
        for bad in (1, MULTI_MAX + 1, -1):
            assert wide(bad) < 0
            assert b"coalesce" in L.smartgpu_last_error()
        assert wide(32) == 32  # a refused value changed nothing
        # the narrow call: the same number, a wider previous value reported as 8
        assert narrow(8) == 8
        assert wide(20) == 8
        assert narrow(9) < 0 and b"coalesce" in L.smartgpu_last_error()
        assert wide(20) == 20  # refused: nothing changed
        assert narrow(0) == 8
        assert wide(5) == 0
        assert narrow(5) == 5
        for g in (2, 8):
            wide(g)
            assert narrow(g) == g
    finally:
        wide(default)
    assert wide(default) == default


def test_product_library_exports_the_wide_call():
    L = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(L, "smartgpu_coalesce_wide")
    assert "coalesce_wide" in dir(engine)
