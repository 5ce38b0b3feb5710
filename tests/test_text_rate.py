"""How often two symbols of a text are equal, without a device.

tests/text_rate_check.cpp includes smart_amd/csrc/text_rate.hpp alone (the header is free of HIP) and checks the rate
function on histograms: uniform over 128, 48 and 32 values at N = 2^22 (1/128, 1/48, 1/32 to within 1e-6, and the closed
form to the last bit), a single value (1), 256 different bytes (0), N = 0 and N = 1 (no rate), counts of 2^32 - 1 and
2^33 (c (c - 1) near and beyond 2^64); the side of 1/48 a rate lies on; and the sample a text of n bytes gives — whole up
to 16 MiB, 2^20 chunks at an even stride beyond, every chunk inside the text.  The program is compiled with
AddressSanitizer and UBSan and runs as a program, without a preload.

The two calls that report what the launch queue does with it are part of the ABI."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

from smart_amd import engine

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("text_rate") / "text_rate_check"
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "text_rate_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    return str(exe)


def test_rate_of_a_histogram_and_the_sample_of_a_text(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # 3 uniform x 2, 3 on the side of 1/48, 3 single values, all different, N = 0, N = 1, 2 large counts, 10 + 8 samples
    assert r.returncode == 0 and failures == 0 and cases == 6 + 3 + 3 + 1 + 2 + 2 + 18, r.stdout[-4000:] + r.stderr[-2000:]


def test_product_library_exports_the_two_calls():
    L = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(L, "smartgpu_text_repeat_rate") and hasattr(L, "smartgpu_coalesce_riders")
    assert "coalesce_riders" in dir(engine) and hasattr(engine.Text, "repeat_rate")


def test_riders_of_a_device_that_was_never_used():
    engine.build()
    assert engine.coalesce_riders(0) >= 0
    n = ctypes.c_uint64(0)
    assert engine.lib().smartgpu_coalesce_riders(-1, ctypes.byref(n)) < 0 and engine.lib().smartgpu_coalesce_riders(0, None) < 0
    rate = ctypes.c_double(0.0)
    assert engine.lib().smartgpu_text_repeat_rate(None, ctypes.byref(rate)) < 0
