"""The dispatcher against itself, on the CPU: launch.hip holds no kernel and makes no HIP call — it only calls the
launch_* functions of launch_common.hpp — so it links against stubs that record their call (tests/dispatch_driver.cpp).

For all 16 algorithms, m in {1..40, 47, 48, 63, 64, 65, 255, 256, 4096}, the plan words build_blob produces for rand2,
rand4, English and rand128 patterns of that length, the three kinds of text codes (none, four values, two values) and
every smartgpu_tune setting the build accepts for the keys launch.hip reads:

* launch_scan makes exactly one launch, and scan_kernel_name names the kernel that launch runs (the gram launchers
  count as their base kernel) — an invariant, not a recorded table: retuning a threshold does not touch this test;
* plans of one algorithm and length with equal group_key lead to the same launcher with the same argument and the
  same launcher-read words — what a pattern set that runs as one grid relies on.

The driver links the plan builder (plan.cpp) itself and asserts, for every blob of that grid, the layout facts the kernels
rely on without checking: size and pattern slot, the place and contents of the Shift-Or masks of a rerouted plan, room
for the algorithm's own tables where kernels.hpp states their place, and that a build into a reused vector equals a
build into a fresh one.  All of it is compiled with AddressSanitizer and UBSan and runs as a program, without a preload."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "smart_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-result", "-Wno-unused-value", "-Wno-unused-function"] + SANITIZE


@pytest.mark.parametrize("build", ["product", "ab"])
def test_kernel_name_is_the_launcher_launch_scan_calls(tmp_path, build):
    define = ["-DSMARTGPU_AB"] if build == "ab" else []
    units = {"plan": os.path.join(CSRC, "plan.cpp"), "launch": os.path.join(CSRC, "launch.hip"), "tables": os.path.join(CSRC, "tables.cpp"),
             "driver": os.path.join(ROOT, "tests", "dispatch_driver.cpp")}
    procs = [(u, subprocess.Popen([HIPCC] + FLAGS + define + ["--offload-arch=gfx950", "-c", "-o", str(tmp_path / (u + ".o")), src],
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for u, src in units.items()]
    for u, p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, (u, out)
    exe = tmp_path / "dispatch_driver"
    subprocess.check_call([HIPCC, "-o", str(exe)] + SANITIZE + [str(tmp_path / (u + ".o")) for u in units] + ["-ldl"])
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "english_excerpt.txt")], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) grid points, (\d+) pairs, (\d+) tune settings, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-2000:]
    points, pairs, tunes, failures = map(int, summary.groups())
    assert r.returncode == 0 and failures == 0, r.stdout[-4000:]
    # 16 algorithms x 48 lengths less the inapplicable ones, x 4 patterns x 3 kinds of codes x the tune settings
    assert tunes >= (24 if build == "product" else 288) and points >= 9000 * tunes and pairs == points // 4 * 6
