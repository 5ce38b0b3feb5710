"""Positions of a pattern set on a byte text (smartgpu_find_batch64, hor_multi_find) without a GPU: the declaration and the
export, the published widths and bounds, the source registry, the refusals that are decided before the first HIP call, the
ordering of mixed lengths in the Python wrapper (the C call stubbed), and the host ordering and a CPU model of the kernel's
walk (tests/find_batch_check.cpp), compiled by the host compiler plain and under AddressSanitizer / UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

ERR_ARG = -3


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


# ---- declaration, export, registry ---------------------------------------------------------------------------------------

def test_header_declares_the_call_and_both_libraries_export_it():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+smartgpu_find_batch64\s*\(const uint8_t \*const \*P, uint32_t m, uint32_t K, const smartgpu_text \*text,", code)
    assert re.search(r"^#define\s+SMARTGPU_FIND_BATCH_STAGING\s+\(32u << 20\)", code, flags=re.M)
    for path in (engine.LIB_PATH, engine.AB_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "smartgpu_find_batch64"), path
        f = engine._load(path).smartgpu_find_batch64
        assert f.restype is ctypes.c_int and len(f.argtypes) == 9, path
    for name in ("find_batch", "find_width", "find_batch_max"):
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_and_makefile_hold_the_unit():
    assert sources.KERNEL_UNIT["hor_multi_find"] == "k_hormf"
    assert sources.UNITS["k_hormf"] == ("k_hormf.hip", "multi_find.hpp", "multi.hpp")
    for f in sources.UNITS["k_hormf"]:
        assert os.path.exists(os.path.join(sources.CSRC, f)), f
    assert sources.kernel_sha256("hor_multi_find") == sources.unit_sha256("k_hormf") != sources.unit_sha256("k_horm")
    assert sources.UNITS["k_horm"] == ("k_horm.hip", "multi.hpp") and sources.KERNEL_UNIT["hor_multi_scan"] == "k_horm"
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_hormf\b", makefile, flags=re.M)
    for header in ("multi_find.hpp", "multi_find_host.hpp"):
        assert re.search(r"^HEADERS\s*:=.*\b%s\b" % re.escape(header), makefile, flags=re.M), header
    unit = open(os.path.join(sources.CSRC, "k_hormf.hip")).read()
    assert not re.search(r'#include\s+"k_', unit) and re.search(r'#include\s+"multi_find.hpp"', unit)
    assert "asm" not in re.sub(r"//.*", "", unit)  # no inline assembly
    host = open(os.path.join(sources.CSRC, "multi_find_host.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", host).lower() and "set_error" not in host  # host only: no HIP call, no error text


# ---- the published widths and the K bound ----------------------------------------------------------------------------------

def _lds_width(m):
    """The widest pass whose workgroup takes at most 40960 bytes of LDS (four per CU), counted as multi_find.hpp says: the
    table, the heads, a row, a link and a sum per pattern (rounded to 64), the stage, the tile."""
    stride = (min(m, 65) + 15) // 16 * 16
    stage = 8 * 128 + 64
    tile = (48 + 16384 + 16 + 63) // 64 * 64
    np_ = 0
    while True:
        k = np_ + 1
        lds = 16384 + 4 * 512 + (k * (stride + 8) + 63) // 64 * 64 + stage + tile
        if k > 256 or k * stride > 2 * 256 * 16 or lds > 40960:
            return np_
        np_ = k


def test_widths_and_bound_hold_as_documented():
    lengths = (3, 4, 8, 16, 17, 18, 32, 33, 48, 49, 64, 65, 100, 300, 4096)
    assert [engine.find_width(m) for m in lengths] == [_lds_width(m) for m in lengths]
    assert [engine.find_width(m) for m in (16, 32, 48, 64, 65)] == [208, 124, 89, 69, 56]
    hpp = open(os.path.join(sources.CSRC, "multi_find.hpp")).read()
    assert re.search(r"find_width\(3\) == 208 && find_width\(16\) == 208 && find_width\(17\) == 124 && find_width\(32\) == 124 && find_width\(33\) == 89", hpp)
    assert re.search(r"find_width\(49\) == 69 && find_width\(64\) == 69 && find_width\(65\) == 56 && find_width\(4096\) == 56", hpp)
    assert re.search(r"constexpr uint32_t kFindBatchShift = 18;", hpp) and re.search(r"constexpr uint32_t kFindStage = 128;", hpp)
    # the K bound: the staging buffer over the bytes staged per pattern, 2^18 at the most
    assert engine.FIND_BATCH_MAX_K == 1 << 18 and engine.FIND_BATCH_STAGING == 32 << 20
    for m, per in ((3, 16), (16, 16), (17, 32), (18, 32 + 32), (32, 32 + 32), (64, 64 + 64), (65, 80 + 80), (300, 80 + 304), (4096, 80 + 4096)):
        assert engine.find_batch_max(m) == min((32 << 20) // per, 1 << 18), m
    assert engine.find_batch_max(300) == 87381 and engine.find_batch_max(4096) == 8035 and engine.find_batch_max(64) == 1 << 18
    assert re.search(r"find_batch_max\(300\) == 87381 && find_batch_max\(4096\) == 8035", hpp)
    header = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    assert "87381 patterns at m = 300, 8035 at m = 4096" in header and "208 patterns up to m = 16, 124 up to m = 32, 89 up to m = 48, 69 up to" in header


# ---- refusals that need no device ------------------------------------------------------------------------------------------

def _refused(rc, says):
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


def test_refusals_that_need_no_device():
    """Without a device there is no text handle: every call below is decided before the first HIP call."""
    f = engine.lib().smartgpu_find_batch64
    pat = np.arange(32, dtype=np.uint8)
    ptrs = (ctypes.c_void_p * 2)(pat.ctypes.data, pat.ctypes.data)
    P = ctypes.cast(ptrs, ctypes.c_void_p)
    out = np.zeros(8, dtype=np.uint64)
    starts = np.full(3, 77, dtype=np.uint64)
    _refused(f(None, 32, 2, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data), "find_batch: P/starts NULL or K = 0")
    _refused(f(P, 32, 0, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data), "find_batch: P/starts NULL or K = 0")
    _refused(f(P, 32, 2, None, 0, 100, out.ctypes.data, 8, None), "find_batch: P/starts NULL or K = 0")
    _refused(f(P, 32, (1 << 18) + 1, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data), "262145 patterns in one set (at most 262144")
    _refused(f(P, 5000, 2, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data), "pattern length 5000 outside [1,")
    _refused(f(P, 32, 2, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data), "text handle is NULL")
    assert starts.tolist() == [77, 77, 77] and not out.any()  # a refused call writes nothing


def test_the_checks_come_before_the_first_device_call():
    api = open(os.path.join(sources.CSRC, "api.cpp")).read()
    body = api[api.index("int smartgpu_find_batch64("):]
    body = body[:body.index("\n}\n")]
    order = [body.index(s) for s in ("P/starts NULL or K = 0", "patterns in one set", "check_search_args(", "positions NULL with cap > 0", "pattern %u is NULL",
                                     "sg::find_batch_max(m)", "sg::kFindBatchMaxEnd", "if (m > n) return SMARTGPU_OK", "device_ctx_flushed(")]
    assert order == sorted(order)
    assert body.count("device_ctx_flushed(") == 1 and "hor_multi_find: cursor %llu" in body and "order_find_batch(" in body


# ---- the Python wrapper ------------------------------------------------------------------------------------------------

def test_find_batch_rejects_an_empty_set():
    with pytest.raises(engine.SmartGpuError, match="empty pattern set"):
        engine.find_batch([], None, n=0)


def test_find_batch_orders_mixed_lengths_back(monkeypatch):
    """Patterns of three lengths in one set: one call per length, the results in the caller's order, `cap` the room for all
    lengths together (the C call stubbed: a pattern b"x" * m 'occurs' at m, 2m, .. m * first byte)."""
    calls = []

    def stub(pats, text, off, n, cap):
        calls.append(([bytes(p) for p in pats], cap))
        lists = [np.arange(1, int(p[0]) + 1, dtype=np.uint64) * len(p) for p in pats]
        counts = np.array([len(x) for x in lists], dtype=np.uint64)
        return (lists if int(counts.sum()) <= cap else None), counts

    monkeypatch.setattr(engine, "_find_batch_one", stub)
    pats = [bytes([3]) * 5, bytes([1]) * 2, bytes([2]) * 5, bytes([4]) * 9, bytes([0]) * 2]
    lists, counts = engine.find_batch(pats, None, n=1000, cap=10)
    assert counts.tolist() == [3, 1, 2, 4, 0]
    assert [x.tolist() for x in lists] == [[5, 10, 15], [2], [5, 10], [9, 18, 27, 36], []]
    # one call per length, each with the room the earlier ones left
    assert calls == [([pats[1], pats[4]], 10), ([pats[0], pats[2]], 9), ([pats[3]], 4)]
    # one entry too few: None, and every count — the later lengths are still counted
    calls.clear()
    lists, counts = engine.find_batch(pats, None, n=1000, cap=5)
    assert lists is None and counts.tolist() == [3, 1, 2, 4, 0]
    assert [c[1] for c in calls] == [5, 4, 0]


# ---- the ordering and the walk on the CPU ------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True])
def test_ordering_and_walk_on_the_host(tmp_path, sanitize):
    """tests/find_batch_check.cpp by the host compiler, plain and with AddressSanitizer and UBSan, run as a child process:
    order_find_batch over shuffled entries of a naive search (duplicate patterns, empty slices, every refusal), and the
    model of the kernel's walk — table, halo, chains, stage of 1 and of 4 entries, three passes on one cursor — against
    the naive (s, k) set for m in {3, 4, 16, 17, 18, 33, 65, 300} on texts of 2, 128, 256 values and of one."""
    exe = tmp_path / "find_batch_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "find_batch_check.cpp")]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # the ordering: 8 checks; the walk: 4 texts x 8 lengths x 2 stage sizes
    assert r.returncode == 0 and failures == 0 and cases == 8 + 4 * 8 * 2, r.stdout[-4000:] + r.stderr[-2000:]
