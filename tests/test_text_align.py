"""Starts and alignments of edit-distance occurrences on BYTE texts (smartgpu_align_edit64, smartgpu_align_edit_classes64)
without a GPU: the declarations and bindings of both libraries, the source registry, the documents, the refusals that are
decided before the first HIP call, the hand example held to the by-definition oracle of tests/test_packed_align.py
(align_one), the shared headers on the CPU under sanitizers (tests/text_align_check.cpp), and the compiled kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

from test_packed_align import align_one, pack_ops
from test_packed_edit import byte_accepts

SYMBOLS = {"smartgpu_align_edit64": 11, "smartgpu_align_edit_classes64": 11}
PYTHON = ("align_edit", "align_edit_classes", "find_edit_align", "find_edit_classes_align")
ERR_ARG = -3

# The hand example: (pattern, k, {end: (start, distance, cigar)}) on HAND_TEXT; tests/test_text_align_gpu.py holds the library to it.
HAND_TEXT = b"Did you recieve the mesage? I beleive so."
HAND = (
    (b"receive", 2, {12: (8, 2, "3=1D1=1D1="), 14: (8, 2, "3=2X2="), 36: (31, 2, "1D1=1X4=")}),
    (b"message", 1, {25: (20, 1, "3=1D3=")}),
    (b"believe", 2, {14: (9, 2, "1D1=1X4="), 36: (30, 2, "3=2X2=")}),
)


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


# ---- declarations, bindings, registry, documents -----------------------------------------------------------------------

def test_header_declares_the_calls():
    raw = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    assert "start positions or alignments" not in raw
    assert "NOT offered: the longest start, all starts, all optimal alignments" in raw
    # the byte-text edit calls no longer disclaim starts and alignments, the packed align calls no longer disclaim byte texts
    assert "7, start positions and alignments, Hamming-only" not in raw
    assert "affine costs, byte texts, a kernel" not in raw
    assert "k_talign.hip" in raw and "tools/talign_probe.py" in raw


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
    with pytest.raises(ValueError):  # the classes forms go through _classes: the shape is checked before any call
        smart_amd.align_edit_classes(np.zeros((4, 31), dtype=np.uint8), None, 1, [3])
    with pytest.raises(ValueError):
        smart_amd.find_edit_classes_align(np.zeros(32, dtype=np.uint8), None, 1)


def test_sources_registry_has_the_unit_and_leaves_the_other_units_alone():
    assert [f for f in sources.UNITS["k_talign"] if f.startswith("k_")] == ["k_talign.hip"]
    for f in ("talign.hpp", "talign_host.hpp", "tedit_host.hpp", "edit_align.hpp", "edit_step.hpp"):
        assert f in sources.UNITS["k_talign"], f
        assert os.path.exists(os.path.join(sources.CSRC, f)), f
    assert sources.KERNEL_UNIT["text_edit_align"] == "k_talign"
    sha = sources.unit_sha256("k_talign")
    assert sources.kernel_sha256("text_edit_align") == sha and sha not in (sources.unit_sha256("k_tedit"), sources.unit_sha256("k_palign"))
    assert sources.UNITS["k_tedit"] == ("k_tedit.hip", "text_tile.hpp", "tedit.hpp", "tedit_host.hpp", "edit_step.hpp", "planes.hpp")
    assert sources.UNITS["k_palign"] == ("k_palign.hip", "palign.hpp", "edit_align.hpp", "pedit.hpp", "pedit_host.hpp", "edit_step.hpp", "planes.hpp")
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_talign\b", makefile, flags=re.M)
    for h in ("talign.hpp", "talign_host.hpp"):
        assert re.search(r"^HEADERS\s*:=.*\$\(HERE\)%s\b" % re.escape(h), makefile, flags=re.M), h


def test_documents_name_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + list(PYTHON):
        assert n in doc, n
    assert "smartgpu_align_edit64" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "text_edit_align" in design and "k_talign.hip" in design
    results = open(os.path.join(ROOT, "profiles", "tedit", "RESULTS.md")).read()
    assert "Starts and alignments" in results and "talign_probe.py" in results
    assert os.path.exists(os.path.join(ROOT, "tools", "talign_probe.py"))


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_classes"])
def test_refusals_that_need_no_device(kind):
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call, for
    the reason its line states, and writes nothing.  (An end outside a REAL range is refused in tests/test_text_align_gpu.py.)"""
    f = getattr(engine.lib(), "smartgpu_align_edit%s64" % kind)
    P = np.full(32 * 100, 1, dtype=np.uint8)
    ends = np.arange(8, dtype=np.uint64)
    starts = np.full(8, 77, dtype=np.uint64)
    dist = np.full(8, 7, dtype=np.uint8)
    ops = np.full(24, 5, dtype=np.uint64)
    call = lambda p, m, k, e, cnt, s: f(p, m, k, None, 0, 100, e, cnt, s, dist.ctypes.data, ops.ctypes.data)  # noqa: E731
    _refused(call(None, 4, 1, ends.ctypes.data, 8, starts.ctypes.data), "classes is NULL" if kind else "P is NULL")
    _refused(call(P.ctypes.data, 0, 1, ends.ctypes.data, 8, starts.ctypes.data), "length 0 outside [1,64]")
    _refused(call(P.ctypes.data, 65, 1, ends.ctypes.data, 8, starts.ctypes.data), "length 65 outside [1,64]")
    _refused(call(P.ctypes.data, 4, 8, ends.ctypes.data, 8, starts.ctypes.data), "k = 8 edits, at most 7")
    _refused(call(P.ctypes.data, 4, 1, None, 8, starts.ctypes.data), "ends NULL with count > 0")
    _refused(call(P.ctypes.data, 4, 1, ends.ctypes.data, 8, None), "starts NULL with count > 0")
    _refused(call(P.ctypes.data, 4, 1, ends.ctypes.data, 8, starts.ctypes.data), "text handle is NULL")
    _refused(call(P.ctypes.data, 4, 1, None, 0, None), "text handle is NULL")  # count == 0 excuses the NULL lists, not the NULL text
    assert ("align_edit%s64:" % kind) in engine.lib().smartgpu_last_error().decode()
    assert (starts == 77).all() and (dist == 7).all() and (ops == 5).all() and (ends == np.arange(8)).all()


# ---- the hand example ----------------------------------------------------------------------------------------------------

def test_the_hand_example_is_what_the_oracle_says():
    """The strings a reader can check by eye ARE the definition's: align_one with byte_accepts gives exactly them."""
    T = np.frombuffer(HAND_TEXT, dtype=np.uint8)
    for word, k, want in HAND:
        P = np.frombuffer(word, dtype=np.uint8)
        for e, (s, d, cigar) in want.items():
            got = align_one(len(P), byte_accepts(P), T, e, k)
            assert got is not None and got[:2] == (s, d), (word, e, got)
            assert smart_amd.edit_cigar(np.array(pack_ops(got[2]), dtype=np.uint64)) == cigar, (word, e)


# ---- the shared headers on the CPU ---------------------------------------------------------------------------------------

def test_window_reversal_step_and_traceback_on_the_host(tmp_path):
    """tests/text_align_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process: talign_host.hpp and
    edit_align.hpp fed as the kernel feeds them — the 256-mask table of the reversed pattern, bytes from the dword window at
    every e % 4 — against a scalar DP written out in the program: start, distance, every operation and the packing."""
    exe = tmp_path / "text_align_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "text_align_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # per length: 4 alphabets x 2 kinds of pattern x 4 values of k x (every end of the text + the walks clipped at off),
    # + (both kinds of end and every phase seen) + the full rows + the empty rows; 4 lengths on one dword, 7 on two
    assert r.returncode == 0 and failures == 0 and cases == (4 + 7) * (4 * 2 * 4 * 2 + 3), r.stdout[-4000:] + r.stderr[-2000:]


def test_the_unit_holds_four_kernels_without_scratch_within_64_kb_of_lds():
    """text_edit_align for one and two mask dwords, with and without the traceback: exactly four kernels of the k_talign code
    object, each with ScratchSize 0 (-Rpass-analysis=kernel-resource-usage).  The LDS is static, so the compiler reports all
    of it, and the launcher asks for no more: table + window + columns, the geometry of the kernel restated here."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_talign.hip")]
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
    assert len([k for k in usage if "text_edit_align" in k]) == 4, sorted(usage)
    text = open(os.path.join(sources.CSRC, "k_talign.hip")).read()
    assert re.search(r"kLanes = \(WORDS == 2 && OPS\) \? 32 : 64;", text) and re.search(r"kCols = WORDS == 2 \? 72 : 40;", text)
    assert re.search(r"hipLaunchKernelGGL\(\(text_edit_align<w_, o_>\), dim3\(\(uint32_t\)grid\), dim3\(G::kLanes\), 0, stream, a\);", text)  # no dynamic LDS
    for words in (1, 2):
        for ops in (0, 1):
            mine = [k for k in usage if re.search(r"text_edit_alignILi%dELb%dEE" % (words, ops), k)]
            assert len(mine) == 1, (words, ops, sorted(usage))
            lanes = 32 if words == 2 and ops else 64
            window = 1 + (32 * words + 7 - 1 + 3) // 4  # aligned dwords that hold m + k <= 32 * words + 7 bytes ending anywhere in a dword
            assert window == (11, 19)[words - 1]
            lds = 4 * (256 * words + window * lanes + ((40, 72)[words - 1] * 2 * words * lanes if ops else 0))
            assert lds <= 65536
            assert usage[mine[0]] == {"scratch": 0, "lds": lds}, (mine[0], usage[mine[0]], lds)
