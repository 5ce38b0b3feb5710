"""Long passes of hor_multi_scan without a device.

A long pass (smart_amd/csrc/multi.hpp: long_width) carries two pointers per pattern and reads its rows from the plans'
blobs, so it takes what the LDS of a workgroup has room for at four workgroups per CU, not what the kernel's arguments
hold by value: 252 patterns up to m = 16, 152 up to m = 32, 108 up to 48, 84 up to 64, 68 beyond.

tests/coalesce_long_check.cpp gathers the rows of a long pass in 16-byte pieces from pattern slots whose bytes behind the
pattern are NOT zero, into a heap buffer laid out as the kernel's LDS, builds the byte table and the chains, walks 512 KiB
of rand128 and rand256 and compares every count with brute force, at m = 8, 16, 17, 32, 33, 64, 65 and 100: the by-value
pass of pass_width(m), the long pass of long_width(m), the narrowest long pass (pass_width(m) + 1), and a long pass with
planted copies — one pattern at a place below and a place beyond pass_width(m), two patterns of one last gram, the last
place, a periodic run.  It prints the wave-steps per 4096 bytes and the share of steps that hit a slot at both widths
(profiles/coalesce/RESULTS.md has them beside the GPU's figures).  Compiled with AddressSanitizer and UBSan; it runs as a
program, without a preload.

The setting: smartgpu_coalesce_long takes -1 (no long passes) and any range from 0 bytes on, returns the previous value,
refuses anything below -1 with a message and changes nothing then; the three calls that set the pass width neither
change it nor are changed by it."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

from smart_amd import engine

HIPCC = "/opt/rocm/bin/hipcc"
MS = (3, 8, 16, 17, 32, 33, 48, 49, 64, 65, 66, 100, 256, 4096, 4200)


def stride(m):
    """multi.hpp tail_stride: the bytes of a row, min(m, 65) rounded to 16"""
    return (min(m, 65) + 15) // 16 * 16


def long_width(m):
    """The largest np with 16 np <= 4032, np <= 256 - 4 and 16384 + 4 * 512 + 8 np + round64(np * stride) + 16448 <= 40960."""
    fits = [np for np in range(1, 300) if 16 * np <= 4032 and np <= 252 and 16384 + 2048 + 8 * np + ((np * stride(m) + 63) & ~63) + 16448 <= 40960]
    assert fits == list(range(1, len(fits) + 1))  # what fits is an interval from 1
    return fits[-1]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("coalesce_long") / "coalesce_long_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "coalesce_long_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    return str(exe)


def test_long_pass_on_the_host_counts_like_brute_force(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # 2 texts x 8 lengths x (by value, long, the narrowest long pass, the long pass with the planted copies)
    assert r.returncode == 0 and failures == 0 and cases == 2 * 8 * 4, r.stdout[-4000:] + r.stderr[-2000:]
    # the model's figures are there for every text and length, at both widths
    rows = re.findall(r"^(rand\d+) +m +(\d+): np +(\d+) ([\d.]+) wave-steps per 4096 bytes, ([\d.]+) % of steps hit \| np +(\d+) ([\d.]+), ([\d.]+) %$", r.stdout, re.M)
    assert [(t, int(m)) for t, m, *_ in rows] == [(t, m) for t in ("rand128", "rand256") for m in (8, 16, 17, 32, 33, 64, 65, 100)]
    for _, m, w, _, _, lw, _, _ in rows:
        assert int(w) == engine.pass_width(int(m)) and int(lw) == engine.long_width(int(m))


def test_long_width_follows_the_formula():
    assert [engine.long_width(m) for m in MS] == [long_width(m) for m in MS]
    assert [engine.long_width(m) for m in (16, 17, 32, 33, 48, 49, 64, 65, 4200)] == [252, 152, 152, 108, 108, 84, 84, 68, 68]
    for m in range(3, 300):
        assert engine.long_width(m) == long_width(m) > engine.pass_width(m)
        assert 16 * engine.long_width(m) <= 4032


def test_the_setting_round_trip():
    L = engine.lib()
    f = L.smartgpu_coalesce_long
    default = f(0)
    try:
        assert default == engine.LONG_DEFAULT == 64 << 20
        prev = 0
        for v in (0, 1, -1, 0, 64 << 20, 1 << 40, -1, -1, 8 << 20):
            assert f(v) == prev
            prev = v
        for bad in (-2, -3, -(1 << 40)):
            assert f(bad) == -3  # SMARTGPU_ERR_ARG
            err = L.smartgpu_last_error()
            assert b"coalesce_long" in err and b"-1" in err and str(bad).encode() in err
            assert f(8 << 20) == 8 << 20  # a refused value changed nothing
        assert engine.coalesce_long(-1) == 8 << 20
        assert engine.coalesce_long(0) == -1
        with pytest.raises(Exception):
            engine.coalesce_long(-2)
        assert engine.coalesce_long(0) == 0
    finally:
        f(default)
    assert f(default) == default


def test_the_width_calls_and_the_long_setting_leave_each_other_alone():
    L = engine.lib()
    full, wide, narrow, long_ = L.smartgpu_coalesce_pass, L.smartgpu_coalesce_wide, L.smartgpu_coalesce, L.smartgpu_coalesce_long
    width, least = full(96), long_(0)
    try:
        for v in (-1, 0, 1 << 30):
            long_(v)
            assert full(96) == 96 and wide(32) == 32 and full(96) == 32 and narrow(8) == 8 and full(0) == 8 and full(96) == 0
            assert full(97) < 0 and b"2..96" in L.smartgpu_last_error()
            assert long_(v) == v  # no width call moved it
        assert engine.pass_width(32) == 84 and engine.PASS_MAX == 96
    finally:
        full(width)
        long_(least)


def test_product_library_exports_the_call():
    L = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(L, "smartgpu_coalesce_long")
    assert "coalesce_long" in dir(engine) and "long_width" in dir(engine)
