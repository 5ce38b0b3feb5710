"""Edit distance for long patterns on packed texts (smartgpu_psearch_editl64, smartgpu_pfind_editl64 and their sets forms)
without a GPU: the declarations and bindings of both libraries, the source registry, the documentation, the refusals that
are decided before the first HIP call, the block recurrence and its cut-off on the CPU under sanitizers
(tests/packed_editl_check.cpp), and the compiled kernels.  The oracle of the GPU tests is tests/test_packed_edit.py's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_psearch_editl64": 10, "smartgpu_pfind_editl64": 11, "smartgpu_psearch_sets_editl64": 10, "smartgpu_pfind_sets_editl64": 11}
CONSTANTS = {"SMARTGPU_PEDITL_MAXM": "256", "SMARTGPU_PEDITL_MAXK": "31", "SMARTGPU_PEDITL_ALL_BLOCKS": "1u"}
PYTHON = ("psearch_editl", "pfind_editl", "psearch_sets_editl", "pfind_sets_editl")
ERR_ARG = -3
# what k_peditl.hip chose (peditl.hpp kEditlRun, kEditlPiece; test_the_restated_run_length_is_the_kernels): end positions a
# lane owns, the piece it loads at a time, and with the run those of a wave (64 lanes) and of a workgroup (256 lanes)
RUN = 512
PIECE = 128
WAVE_RUN = 64 * RUN
WG_RUN = 256 * RUN


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def test_header_declares_the_calls_and_the_constants():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define\s+%s\s+%s\s*$" % (name, value), text, flags=re.M), name
    assert re.search(r"^#define\s+SMARTGPU_PEDIT_MAXM\s+64\b", text, flags=re.M)  # the existing calls keep their bound


def test_both_libraries_export_and_bind_them():
    for path in (engine.LIB_PATH, engine.AB_LIB_PATH):
        raw = ctypes.CDLL(path)
        L = engine._load(path)
        for n, nargs in SYMBOLS.items():
            assert hasattr(raw, n), (path, n)
            f = getattr(L, n)
            assert f.argtypes is not None and f.restype is ctypes.c_int, (path, n)
            assert len(f.argtypes) == nargs, (path, n)


def test_python_functions_exist():
    for name in PYTHON:
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_has_the_unit_and_leaves_the_other_units_alone():
    assert [f for f in sources.UNITS["k_peditl"] if f.startswith("k_")] == ["k_peditl.hip"]
    for f in ("peditl.hpp", "peditl_host.hpp", "edit_block.hpp"):
        assert f in sources.UNITS["k_peditl"], f
    for k in ("planes_editl_scan", "planes_editl_find"):
        assert sources.KERNEL_UNIT[k] == "k_peditl"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_peditl") != sources.unit_sha256("k_pedit")
    assert sources.UNITS["k_pedit"] == ("k_pedit.hip", "pedit.hpp", "pedit_host.hpp", "edit_step.hpp", "planes.hpp")
    assert sources.UNITS["k_palign"] == ("k_palign.hip", "palign.hpp", "edit_align.hpp", "pedit.hpp", "pedit_host.hpp", "edit_step.hpp", "planes.hpp")
    assert sources.UNITS["k_planes"] == ("k_planes.hip", "planes.hpp")
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_peditl\b", makefile, flags=re.M)
    for h in ("peditl.hpp", "peditl_host.hpp", "edit_block.hpp"):
        assert re.search(r"^HEADERS\s*:=.*\b%s\b" % re.escape(h), makefile, flags=re.M), h


def test_the_restated_run_length_is_the_kernels():
    text = open(os.path.join(sources.CSRC, "peditl.hpp")).read()
    assert re.search(r"constexpr uint32_t kEditlRun = %d;" % RUN, text)
    assert re.search(r"constexpr uint32_t kEditlPiece = %d;" % PIECE, text)


def test_documents_name_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + list(PYTHON) + list(CONSTANTS):
        assert n in doc, n
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "smartgpu_psearch_editl64" in readme and "smartgpu_pfind_editl64" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "planes_editl_scan" in design and "planes_editl_find" in design
    header = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    assert "ALIGNMENTS of long patterns" in header  # NOT offered, and said so


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_sets"])
def test_refusals_that_need_no_device(kind):
    """Every call passes a NULL text, so each is decided before the first HIP call, and a refused call writes nothing."""
    L = engine.lib()
    what = "sets is NULL" if kind else "P is NULL"
    P = np.full(300, 1, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    dist = np.zeros(8, dtype=np.uint8)
    c = ctypes.c_uint64(77)
    pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    times = (ctypes.byref(pre), ctypes.byref(run))
    count = getattr(L, "smartgpu_psearch%s_editl64" % kind)
    _refused(count(None, 4, 1, 0, None, 0, 100, ctypes.byref(c), *times), what)
    _refused(count(P.ctypes.data, 0, 1, 0, None, 0, 100, ctypes.byref(c), *times), "length 0 outside [1,256]")
    _refused(count(P.ctypes.data, 257, 1, 0, None, 0, 1000, ctypes.byref(c), *times), "length 257 outside [1,256]")
    _refused(count(P.ctypes.data, 4, 32, 0, None, 0, 100, ctypes.byref(c), *times), "k = 32 edits, at most 31")
    _refused(count(P.ctypes.data, 4, 1, 2, None, 0, 100, ctypes.byref(c), *times), "flags 0x2")
    _refused(count(P.ctypes.data, 4, 1, 3, None, 0, 100, ctypes.byref(c), *times), "flags 0x3")
    _refused(count(P.ctypes.data, 256, 31, 1, None, 0, 100, ctypes.byref(c), *times), "handle is NULL")       # all legal but the handle
    _refused(count(P.ctypes.data, 4, 1, 0, None, 0, 100, None, *times), "handle is NULL")                     # and count == NULL
    assert c.value == 77 and pre.value == -1.0 and run.value == -2.0
    f = getattr(L, "smartgpu_pfind%s_editl64" % kind)
    find = lambda p, m, k, fl, pos, cap, cnt: f(p, m, k, fl, None, 0, 1000, pos, dist.ctypes.data, cap, cnt)  # noqa: E731
    _refused(find(None, 4, 1, 0, out.ctypes.data, 8, ctypes.byref(c)), what)
    _refused(find(P.ctypes.data, 0, 1, 0, out.ctypes.data, 8, ctypes.byref(c)), "length 0 outside [1,256]")
    _refused(find(P.ctypes.data, 257, 1, 0, out.ctypes.data, 8, ctypes.byref(c)), "length 257 outside [1,256]")
    _refused(find(P.ctypes.data, 4, 32, 0, out.ctypes.data, 8, ctypes.byref(c)), "k = 32 edits, at most 31")
    _refused(find(P.ctypes.data, 4, 1, 2, out.ctypes.data, 8, ctypes.byref(c)), "flags 0x2")
    _refused(find(P.ctypes.data, 256, 31, 1, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 0, out.ctypes.data, 8, None), "handle is NULL")                        # and count == NULL
    _refused(find(P.ctypes.data, 4, 1, 0, None, 8, ctypes.byref(c)), "ends NULL")                             # ends == NULL, cap > 0
    assert c.value == 77 and not out.any() and not dist.any()


# ---- the recurrence, the cut-off and the masks on the CPU ----------------------------------------------------------------

def test_block_recurrence_and_cut_off_on_the_host(tmp_path):
    """tests/packed_editl_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process: the recurrence of
    edit_block.hpp on the width the launchers choose against a scalar DP, every column — m = 1, 32, 33, 64, 65, 96, 97, 128,
    129, 255, 256; k = 0, 1, 7, 8, 15, 16, 31; texts on 1 to 4 values; byte patterns (with a copy planted with mixed edits) and
    set patterns; with all blocks (equal in every column), with the cut-off (exact wherever the DP is <= k, above k
    elsewhere), from fresh starts at e - (m + k), and as the kernels run it: 64 lanes in step with one number of active blocks.
    Per length also the all-equal pattern on the all-equal text and, for k = 0, 7, 31, texts with planted prefixes of the
    pattern (31, 32, 33, 64, 100, 200, m - 1 symbols, each followed by a symbol that is not accepted), where the program itself
    asserts that the second block was switched on and, for k <= 7, off again.  And editl_peq_pattern / editl_peq_sets bit by
    bit."""
    exe = tmp_path / "packed_editl_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "packed_editl_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # per length: 4 alphabets x 2 kinds of pattern x 7 budgets x (all blocks, cut-off, fresh starts, the wave) + the all-equal
    # case + 3 budgets of planted prefixes; 11 lengths; the masks: 4 alphabets x 4 lengths x 3 checks
    assert r.returncode == 0 and failures == 0 and cases == 11 * (4 * 2 * 7 * 4 + 1 + 3) + 4 * 4 * 3, r.stdout[-4000:] + r.stderr[-2000:]


def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """planes_editl_scan and planes_editl_find, for one and two planes and 2, 4 and 8 dwords, are kernels of the k_peditl code
    object, each exactly once, with ScratchSize 0 (pv / mv are indexed by constants only) and no static LDS: the scan's 128
    bytes for flush_hits are dynamic, the find uses none."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_peditl.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            usage[cur] = {}
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            usage[cur]["scratch"] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur:
            usage[cur]["lds"] = int(m.group(1))
    for kind in ("scan", "find"):
        for planes in (1, 2):
            for words in (2, 4, 8):
                mine = [k for k in usage if re.search(r"planes_editl_%sILi%dELi%dEE" % (kind, planes, words), k)]
                assert len(mine) == 1, (kind, planes, words, sorted(usage))
                assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
    assert len([k for k in usage if "planes_editl_" in k]) == 12, sorted(usage)
