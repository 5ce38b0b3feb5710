"""A shared pass of up to 96 patterns without a device.

tests/coalesce_pass_check.cpp packs the rows of a pass at the stride of their length, builds the byte skip table, the
bucket heads and the chains of multi.hpp from them, walks 20 000-byte rand128, rand256 and two-symbol periodic texts as
hor_multi_scan does and compares every count with brute force: m = 3, 8, 17, 18, 33, 64, 65, 66, 100; groups of 1, 2,
31, 32, 33, the widest pass of the length and one below it; and, from m = 8 and eight patterns on, a group with two
patterns of one last gram, two patterns of one bucket with different last grams, one pattern twice and a pattern whose
last gram is another's inner gram.  It asserts at compile time the widest pass at m = 16, 17, 32, 64, 65 and the size
of the kernel's arguments.  The program is compiled with AddressSanitizer and UBSan and runs as a program, without a
preload.

The setting: smartgpu_coalesce_pass takes 0 and 2..96 and reports all of it; smartgpu_coalesce_wide reports a wider
value as 32, smartgpu_coalesce as 8; a refused value changes nothing."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

from smart_amd import engine

HIPCC = "/opt/rocm/bin/hipcc"
PASS_MAX = 96


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("coalesce_pass") / "coalesce_pass_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "coalesce_pass_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    return str(exe)


def test_walk_with_byte_table_and_chains_counts_like_brute_force(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # 3 texts x (9 lengths x 7 groups cut from the text + 8 lengths x 5 groups of eight or more with the special patterns)
    assert r.returncode == 0 and failures == 0 and cases == 3 * (9 * 7 + 8 * 5), r.stdout[-4000:] + r.stderr[-2000:]


def test_pass_width_follows_the_row_stride():
    assert engine.PASS_MAX == PASS_MAX
    assert [engine.pass_width(m) for m in (3, 8, 16, 17, 32, 33, 48, 49, 64, 65, 100, 4096)] == [96, 96, 96, 84, 84, 63, 63, 50, 50, 42, 42, 42]


def test_the_three_calls_set_one_number():
    L = engine.lib()
    full, wide, narrow = L.smartgpu_coalesce_pass, L.smartgpu_coalesce_wide, L.smartgpu_coalesce
    default = full(0)
    try:
        assert default == 0 or 2 <= default <= PASS_MAX
        prev = 0
        for g in (2, 8, 9, 32, 33, 64, 84, 95, 96, 0, 96):
            assert full(g) == prev
            prev = g
        for bad in (1, PASS_MAX + 1, -1, 1 << 20):
            assert full(bad) < 0
            err = L.smartgpu_last_error()
            assert b"coalesce" in err and b"2..96" in err and str(bad).encode() in err
            assert full(96) == 96  # a refused value changed nothing
        # the two older calls: the same number, a wider previous value reported as 32 and as 8
        assert wide(32) == 32
        assert full(50) == 32
        assert narrow(8) == 8
        assert full(50) == 8
        assert wide(33) < 0 and b"2..32" in L.smartgpu_last_error()
        assert narrow(9) < 0 and b"2..8" in L.smartgpu_last_error()
        assert full(50) == 50  # refused twice: nothing changed
        assert wide(0) == 32
        assert full(5) == 0
        assert wide(5) == 5 and narrow(5) == 5 and full(5) == 5
    finally:
        full(default)
    assert full(default) == default


def test_product_library_exports_the_full_range_call():
    L = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(L, "smartgpu_coalesce_pass")
    assert "coalesce_pass" in dir(engine)
