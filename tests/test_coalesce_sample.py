"""Sampled passes (hor_sample_scan) without a device.

Next to a text lie the 4 bytes at every 28th position (smart_amd/csrc/sample.hpp); every window of 31 bytes or more
holds one of these grams whole, so a shared pass can filter on the sample and touch the text only where a sampled gram
equals a gram of one of its patterns.

tests/coalesce_sample_check.cpp takes the sample of a text, builds the bit filter, the heads and the entries with the
header's own functions, walks the quads of a range as the kernel does and compares every count with brute force: at
m = 31, 32, 33, 58, 59, 60, 64, 65, 66 and 256, with a copy at every residue of s mod 28, at s = 0 and at s = n - m,
texts of m, m + 1, 55, 56, 57 and 28 k +- 1 bytes, bytes of 128 and more, the same pattern twice, two patterns that agree
in their first 31 bytes, a pattern and its one-byte shift, a run of period 5, and sub-ranges that begin inside a gram.
It is built once plainly and once with AddressSanitizer and UBSan, and runs as a program, without a preload.

The settings: smartgpu_text_sampling takes -1 and any size from 0 on and returns the previous value; it refuses
anything below -1 and changes nothing then.  smartgpu_coalesce_sample is on or off; smartgpu_coalesce_sample_grid takes
0 .. 65536."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

from smart_amd import engine, sources

HIPCC = "/opt/rocm/bin/hipcc"
MS = (31, 32, 33, 58, 59, 60, 64, 65, 66, 256)
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("coalesce_sample_" + request.param) / "coalesce_sample_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall"] + (SANITIZE if request.param == "sanitized" else []) + \
          ["-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "coalesce_sample_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    return str(exe)


def test_sampled_pass_on_the_host_counts_like_brute_force(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # per length: 6 cases per pass width (12 widths in all), rand256, the short texts (25 at m = 31 .. 33, fewer as m grows),
    # equal heads, period 5
    short = sum(len([n for n in [m, m + 1, 55, 56, 57] + [28 * k + d for k in range(2, 12) for d in (-1, 1)] if n >= m]) for m in MS)
    assert r.returncode == 0 and failures == 0 and cases == 6 * 12 + 3 * len(MS) + short, r.stdout[-4000:] + r.stderr[-2000:]
    rows = re.findall(r"^rand128 m +(\d+) np +(\d+): ([\d.]+) % of the samples pass the filter", r.stdout, re.M)
    assert [(int(m), int(np)) for m, np, _ in rows] == [(m, np) for m in MS for np in ((84, 152) if m in (32, 64) else (84,))]
    # 28 np grams in 2^19 bits: about 0.45 % (84) and 0.8 % (152) of samples that belong to no pattern pass by aliasing
    for _, np, rate in rows:
        assert float(rate) < 100.0 * 2 * 28 * int(np) / 2 ** 19, rows


def test_the_constants_and_the_registry():
    assert (engine.SAMPLE_STRIDE, engine.SAMPLE_GRAM, engine.SAMPLE_MIN_M) == (28, 4, 31) and engine.SAMPLE_MIN_M == 28 + 4 - 1
    assert engine.SAMPLE_WIDTH == 4032 // (16 + 32) == 84 and engine.SAMPLE_LONG_WIDTH == 4032 // 16 == 252
    # one CU's LDS holds the widest pass: the filter, the heads, 28 entries of 8 bytes and a sum per pattern
    assert 4 * 2 ** 14 + 4 * 4096 + engine.SAMPLE_LONG_WIDTH * (28 * 8 + 4) <= 160 * 1024
    assert sources.KERNEL_UNIT["hor_sample_scan"] == sources.KERNEL_UNIT["text_sample_build"] == "k_hors"
    assert "k_horm.hip" not in sources.UNITS["k_hors"] and "sample.hpp" in sources.UNITS["k_hors"]
    assert sources.kernel_sha256("hor_sample_scan") != sources.kernel_sha256("hor_multi_scan")
    text = open(os.path.join(ROOT, "smart_amd", "csrc", "k_hors.hip")).read()
    assert "k_horm" not in re.sub(r"//.*", "", text)


def test_the_settings_round_trip():
    L = engine.lib()
    f = L.smartgpu_text_sampling
    default = f(0)
    try:
        assert default == engine.SAMPLING_DEFAULT
        prev = 0
        for v in (0, 1, -1, 0, 64 << 20, 1 << 40, -1, -1, 8 << 20):
            assert f(v) == prev
            prev = v
        for bad in (-2, -(1 << 40)):
            assert f(bad) == -3  # SMARTGPU_ERR_ARG
            err = L.smartgpu_last_error()
            assert b"text_sampling" in err and str(bad).encode() in err
            assert f(8 << 20) == 8 << 20  # a refused value changed nothing
        with pytest.raises(Exception):
            engine.text_sampling(-2)
        assert engine.text_sampling(0) == 8 << 20
    finally:
        f(default)
    width, least = L.smartgpu_coalesce_pass(96), L.smartgpu_coalesce_long(0)
    try:
        assert engine.coalesce_sample(False) is True and engine.coalesce_sample(True) is False and engine.coalesce_sample(True) is True
        assert engine.coalesce_sample_grid(3) == 0 and engine.coalesce_sample_grid(65536) == 3 and engine.coalesce_sample_grid(0) == 65536
        for bad in (-1, 65537):
            with pytest.raises(Exception):
                engine.coalesce_sample_grid(bad)
        assert engine.coalesce_sample_grid(0) == 0
    finally:
        # the other coalesce settings and these leave each other alone
        assert L.smartgpu_coalesce_pass(width) == 96 and L.smartgpu_coalesce_long(least) == 0


def test_product_library_exports_the_calls():
    L = ctypes.CDLL(engine.LIB_PATH)
    for name in ("smartgpu_text_sampling", "smartgpu_text_has_sample", "smartgpu_coalesce_sample", "smartgpu_coalesce_sampled", "smartgpu_coalesce_sample_grid"):
        assert hasattr(L, name), name
