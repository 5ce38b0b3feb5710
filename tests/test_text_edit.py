"""Edit distance on byte texts (smartgpu_search_edit64, smartgpu_find_edit64 and their classes forms) without a GPU: the
declarations and bindings of both libraries, the source registry, the documents, the refusals that are decided before the
first HIP call, byte_classes, the masks, the run geometry and the lanes' fresh starts on the CPU under sanitizers
(tests/text_edit_check.cpp), and the compiled kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_search_edit64": 9, "smartgpu_find_edit64": 10, "smartgpu_search_edit_classes64": 9, "smartgpu_find_edit_classes64": 10}
FUNCTIONS = ("search_edit", "find_edit", "search_edit_classes", "find_edit_classes", "byte_classes")
ERR_ARG = -3


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


# ---- declarations, bindings, registry, documents -----------------------------------------------------------------------

def test_header_declares_the_calls_and_the_bound():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    assert re.search(r"^#define\s+SMARTGPU_EDIT_MAXM\s+64\b", text, flags=re.M)


def test_both_libraries_export_and_bind_them():
    for path in (engine.LIB_PATH, engine.AB_LIB_PATH):
        raw = ctypes.CDLL(path)
        L = engine._load(path)
        for n, nargs in SYMBOLS.items():
            assert hasattr(raw, n), (path, n)
            f = getattr(L, n)
            assert f.argtypes is not None and f.restype is ctypes.c_int, (path, n)  # the engine gave it a prototype
            assert len(f.argtypes) == nargs, (path, n)


def test_python_functions_exist():
    for name in FUNCTIONS:
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_has_the_unit_and_leaves_the_packed_unit_alone():
    assert [f for f in sources.UNITS["k_tedit"] if f.startswith("k_")] == ["k_tedit.hip"]
    for f in ("text_tile.hpp", "tedit.hpp", "tedit_host.hpp", "edit_step.hpp", "planes.hpp"):
        assert f in sources.UNITS["k_tedit"], f
        assert os.path.exists(os.path.join(sources.CSRC, f)), f
    for k in ("text_edit_scan", "text_edit_find"):
        assert sources.KERNEL_UNIT[k] == "k_tedit"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_tedit") != sources.unit_sha256("k_pedit")
    assert sources.UNITS["k_pedit"] == ("k_pedit.hip", "pedit.hpp", "pedit_host.hpp", "edit_step.hpp", "planes.hpp")
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_tedit\b", makefile, flags=re.M)
    for header in ("tedit.hpp", "tedit_host.hpp", "text_tile.hpp"):
        assert re.search(r"^HEADERS\s*:=.*\b%s\b" % re.escape(header), makefile, flags=re.M), header


def test_the_run_length_is_the_packed_kernels():
    """The find's spans are ordered by order_spans, which knows one span length: a lane's run is pedit.hpp's."""
    for header in ("pedit.hpp", "tedit_host.hpp"):
        text = open(os.path.join(sources.CSRC, header)).read()
        assert re.search(r"constexpr uint32_t kT?EditRun = 128;", text), header


def test_documents_name_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + list(FUNCTIONS) + ["SMARTGPU_EDIT_MAXM"]:
        assert n in doc, n
    assert "smartgpu_search_edit64" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "text_edit_scan" in design and "k_tedit.hip" in design
    header = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    assert "tools/tedit_probe.py" in header and os.path.exists(os.path.join(ROOT, "tools", "tedit_probe.py"))


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    """-3 and a message that names the reason (`says`), so that each case is refused for what its comment states."""
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_classes"])
def test_refusals_that_need_no_device(kind):
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call.
    (A range outside a REAL text is refused in tests/test_text_edit_gpu.py; here the NULL handle is what that case meets.)"""
    L = engine.lib()
    what = "classes is NULL" if kind else "P is NULL"
    P = np.full(64 * 32, 1, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    dist = np.zeros(8, dtype=np.uint8)
    c = ctypes.c_uint64(77)
    pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    times = (ctypes.byref(pre), ctypes.byref(run))
    count = getattr(L, "smartgpu_search_edit%s64" % kind)
    name = "search_edit%s64" % kind
    _refused(count(None, 4, 1, None, 0, 100, ctypes.byref(c), *times), what)
    _refused(count(P.ctypes.data, 0, 1, None, 0, 100, ctypes.byref(c), *times), "length 0 outside [1,64]")
    _refused(count(P.ctypes.data, 65, 1, None, 0, 100, ctypes.byref(c), *times), "length 65 outside [1,64]")  # m > SMARTGPU_EDIT_MAXM
    _refused(count(P.ctypes.data, 4, 8, None, 0, 100, ctypes.byref(c), *times), "k = 8 edits, at most 7")      # k > SMARTGPU_PMIS_MAX
    _refused(count(P.ctypes.data, 4, 1, None, 0, 100, ctypes.byref(c), *times), name + ": text handle is NULL")
    _refused(count(P.ctypes.data, 64, 7, None, 1 << 40, 100, ctypes.byref(c), *times), "handle is NULL")       # a range outside the text
    _refused(count(P.ctypes.data, 4, 1, None, 0, 100, None, *times), "handle is NULL")                         # and count == NULL
    assert c.value == 77 and pre.value == -1.0 and run.value == -2.0  # a refused call writes nothing
    f = getattr(L, "smartgpu_find_edit%s64" % kind)
    find = lambda p, m, k, off, n, pos, cap, cnt: f(p, m, k, None, off, n, pos, dist.ctypes.data, cap, cnt)  # noqa: E731
    _refused(find(None, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), what)
    _refused(find(P.ctypes.data, 0, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "length 0 outside [1,64]")
    _refused(find(P.ctypes.data, 65, 1, 0, 5000, out.ctypes.data, 8, ctypes.byref(c)), "length 65 outside [1,64]")
    _refused(find(P.ctypes.data, 4, 8, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "k = 8 edits, at most 7")
    _refused(find(P.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 1 << 40, 100, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, None), "handle is NULL")                    # and count == NULL
    _refused(find(P.ctypes.data, 4, 1, 0, 100, None, 8, ctypes.byref(c)), "ends NULL with cap > 0")            # ends == NULL, cap > 0
    assert c.value == 77 and not out.any() and not dist.any()


def test_the_python_classes_calls_refuse_another_shape():
    for bad in (np.zeros(32, dtype=np.uint8), np.zeros((4, 31), dtype=np.uint8), np.zeros((2, 2, 32), dtype=np.uint8)):
        with pytest.raises(ValueError, match=r"\(m, 32\)"):
            engine.search_edit_classes(bad, None, 1, n=0)


# ---- byte_classes --------------------------------------------------------------------------------------------------------

def bits_of(row):
    return [v for v in range(256) if row[v >> 3] >> (v & 7) & 1]


def test_byte_classes():
    P = np.frombuffer(b"A1z\x00\xff[`@{e", dtype=np.uint8)
    rows = smart_amd.byte_classes(P)
    assert rows.shape == (len(P), 32) and rows.dtype == np.uint8
    for j, v in enumerate(P.tolist()):
        assert bits_of(rows[j]) == [v], j  # one bit per row
    folded = smart_amd.byte_classes(P, ignore_case=True)
    assert bits_of(folded[0]) == [ord("A"), ord("a")]
    assert bits_of(folded[2]) == [ord("Z"), ord("z")] and bits_of(folded[9]) == [ord("E"), ord("e")]
    for j in (1, 3, 4, 5, 6, 7, 8):  # a digit, bytes 0 and 255, and the four neighbours of the letters: ASCII folding only
        assert bits_of(folded[j]) == [int(P[j])], j
    assert bits_of(smart_amd.byte_classes(b"\xc4", ignore_case=True)[0]) == [0xC4]  # nothing beyond 127 folds
    assert smart_amd.byte_classes(b"").shape == (0, 32)


# ---- the masks, the geometry and the lanes' fresh starts on the CPU ------------------------------------------------------

def test_masks_geometry_and_fresh_starts_on_the_host(tmp_path):
    """tests/text_edit_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process: edit_peq_bytes /
    edit_peq_classes bit by bit (bytes 0 and 255, a repeated byte, empty and full rows; m = 1, 31, 32, 33, 64);
    edit_run_walk against a scalar model at both ends of a range, e_begin mid-run and at a run's first and last byte, e_end one
    before, at and one after a multiple of 128 and of 8192, m + k = 1 and 71; and every lane walking its run from a fresh
    start over 40 KiB of 256 values and of 2 values against the full DP (every value <= k equal, every value > k above k)."""
    exe = tmp_path / "text_edit_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "text_edit_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # the masks: 5 lengths x 3 checks; the geometry: 7 range starts x 7 range ends x 2 warm-ups; the walk: 2 texts x 2 lengths
    # x 3 k x 2 ranges
    assert r.returncode == 0 and failures == 0 and cases == 5 * 3 + 7 * 7 * 2 + 2 * 2 * 3 * 2, r.stdout[-4000:] + r.stderr[-2000:]


# ---- the compiled kernels --------------------------------------------------------------------------------------------------

def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """text_edit_scan and text_edit_find, for one and two dwords, are kernels of the k_tedit code object, each with ScratchSize 0
    and no static LDS (-Rpass-analysis=kernel-resource-usage, as tests/test_packed_edit.py reads it)."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_tedit.hip")]
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
        for words in (1, 2):
            mine = [k for k in usage if re.search(r"text_edit_%sILi%dEE" % (kind, words), k)]
            assert len(mine) == 1, (kind, words, sorted(usage))
            assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
