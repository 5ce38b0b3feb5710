"""Mismatches on byte texts (smartgpu_search_mis64, smartgpu_find_mis64 and their classes forms) without a GPU: the
declarations and bindings of both libraries, the source registry, the documents, the refusals that are decided before the
first HIP call, the masks and the lanes' walk on the CPU under sanitizers (tests/text_mis_check.cpp), and the compiled
kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_search_mis64": 9, "smartgpu_find_mis64": 10, "smartgpu_search_mis_classes64": 9, "smartgpu_find_mis_classes64": 10}
FUNCTIONS = ("search_mis", "find_mis", "search_mis_classes", "find_mis_classes")
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
    assert re.search(r"^#define\s+SMARTGPU_MIS_MAXM\s+64\b", text, flags=re.M)


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


def test_sources_registry_has_the_unit_and_leaves_the_edit_unit_alone():
    assert [f for f in sources.UNITS["k_tmis"] if f.startswith("k_")] == ["k_tmis.hip"]
    assert sources.UNITS["k_tmis"] == ("k_tmis.hip", "text_tile.hpp", "tmis.hpp", "tmis_host.hpp", "tedit_host.hpp", "edit_step.hpp", "planes.hpp")
    for f in sources.UNITS["k_tmis"]:
        assert os.path.exists(os.path.join(sources.CSRC, f)), f
    for k in ("text_mis_scan", "text_mis_find"):
        assert sources.KERNEL_UNIT[k] == "k_tmis"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_tmis") != sources.unit_sha256("k_tedit")
    assert sources.UNITS["k_tedit"] == ("k_tedit.hip", "text_tile.hpp", "tedit.hpp", "tedit_host.hpp", "edit_step.hpp", "planes.hpp")
    assert sources.KERNEL_UNIT["text_edit_scan"] == sources.KERNEL_UNIT["text_edit_find"] == "k_tedit"
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_tmis\b", makefile, flags=re.M)
    for header in ("tmis.hpp", "tmis_host.hpp", "text_tile.hpp"):
        assert re.search(r"^HEADERS\s*:=.*\b%s\b" % re.escape(header), makefile, flags=re.M), header


def test_the_new_unit_includes_no_other_kernel_unit_and_shares_the_run_length():
    """k_tmis.hip reads tedit_host.hpp's geometry (the run, edit_run_walk), never k_tedit.hip; the tile and its staging are
    text_tile.hpp's for both units, and neither keeps a copy of the loads."""
    unit = open(os.path.join(sources.CSRC, "k_tmis.hip")).read()
    assert not re.search(r'#include\s+"k_', unit)
    assert "edit_run_walk(c, a.e_begin, a.e_end, top)" in unit  # a warm-up of m - 1 bytes
    for name in ("k_tmis.hip", "k_tedit.hip"):
        text = open(os.path.join(sources.CSRC, name)).read()
        assert re.search(r'#include\s+"text_tile.hpp"', text) and "ld_stream16(" not in text, name
    assert "ld_stream16(" in open(os.path.join(sources.CSRC, "text_tile.hpp")).read()
    assert re.search(r"constexpr uint32_t kTEditRun = 128;", open(os.path.join(sources.CSRC, "tedit_host.hpp")).read())


def test_documents_name_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + list(FUNCTIONS) + ["SMARTGPU_MIS_MAXM"]:
        assert n in doc, n
    readme = open(os.path.join(ROOT, "README.md")).read()
    for n in SYMBOLS:
        assert n in readme, n
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "text_mis_scan" in design and "text_mis_find" in design and "k_tmis.hip" in design and "tmis_host.hpp" in design
    header = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    assert "tools/tmis_probe.py" in header and os.path.exists(os.path.join(ROOT, "tools", "tmis_probe.py"))


def test_the_documents_no_longer_disclaim_hamming_search_on_byte_texts():
    for name in (os.path.join("include", "smartgpu.h"), "README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "Hamming-only search on byte texts" not in text, name
    header = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    # the packed mismatch calls still do not take byte texts, and say where those went
    assert "Byte texts: smartgpu_search_mis64 below" in header and "Byte texts: smartgpu_search_mis_classes64 below" in header
    # what the new calls do not offer is said in the header
    block = header[header.index("MISMATCHES ON A BYTE TEXT"):header.index("#define SMARTGPU_MIS_MAXM")]
    for phrase in ("NOT offered", "m > 64", "k > 7", "a batch call", "MultiText shards", "`smart` harness", "alignments"):
        assert phrase in block, phrase


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    """-3 and a message that names the reason (`says`), so that each case is refused for what its comment states."""
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_classes"])
def test_refusals_that_need_no_device(kind):
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call.
    (A range outside a REAL text is refused in tests/test_text_mis_gpu.py.)"""
    L = engine.lib()
    what = "classes is NULL" if kind else "P is NULL"
    P = np.full(65 * 32, 1, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    dist = np.zeros(8, dtype=np.uint8)
    c = ctypes.c_uint64(77)
    pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    times = (ctypes.byref(pre), ctypes.byref(run))
    count = getattr(L, "smartgpu_search_mis%s64" % kind)
    name = "search_mis%s64" % kind
    _refused(count(None, 4, 1, None, 0, 100, ctypes.byref(c), *times), name + ": " + what)                      # NULL pattern
    _refused(count(P.ctypes.data, 0, 1, None, 0, 100, ctypes.byref(c), *times), name + ": pattern length 0 outside [1,64]")
    _refused(count(P.ctypes.data, 65, 1, None, 0, 100, ctypes.byref(c), *times), name + ": pattern length 65 outside [1,64]")  # m > SMARTGPU_MIS_MAXM
    _refused(count(P.ctypes.data, 4, 8, None, 0, 100, ctypes.byref(c), *times), name + ": k = 8 mismatches, at most 7")        # k > SMARTGPU_PMIS_MAX
    _refused(count(P.ctypes.data, 4, 1, None, 0, 100, ctypes.byref(c), *times), name + ": text handle is NULL")  # NULL text
    _refused(count(P.ctypes.data, 4, 1, None, 0, 100, None, *times), "handle is NULL")                           # and count == NULL
    assert c.value == 77 and pre.value == -1.0 and run.value == -2.0  # a refused call writes nothing
    f = getattr(L, "smartgpu_find_mis%s64" % kind)
    name = "find_mis%s64" % kind
    find = lambda p, m, k, off, n, pos, cap, cnt: f(p, m, k, None, off, n, pos, dist.ctypes.data, cap, cnt)  # noqa: E731
    _refused(find(None, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), name + ": " + what)
    _refused(find(P.ctypes.data, 0, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), name + ": pattern length 0 outside [1,64]")
    _refused(find(P.ctypes.data, 65, 1, 0, 5000, out.ctypes.data, 8, ctypes.byref(c)), name + ": pattern length 65 outside [1,64]")
    _refused(find(P.ctypes.data, 4, 8, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), name + ": k = 8 mismatches, at most 7")
    _refused(find(P.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), name + ": text handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, None), "handle is NULL")                      # and count == NULL
    _refused(find(P.ctypes.data, 4, 1, 0, 100, None, 8, ctypes.byref(c)), name + ": positions NULL with cap > 0")  # positions == NULL, cap > 0
    assert c.value == 77 and not out.any() and not dist.any()


def test_count_null_is_refused_by_name():
    """count == NULL needs a text handle to be reached: tests/host_calls_check.cpp makes one on the CPU and runs the four calls
    through every violation and every pair of two (tests/test_host_calls.py builds it; the driver itself asserts that a pair
    answers as its earlier violation alone, and that a refused call asks for no device and writes nothing)."""
    from test_host_calls import driver_cases
    cases = driver_cases()
    for name in ("search_mis64", "find_mis64", "search_mis_classes64", "find_mis_classes64"):
        find, what = name.startswith("find"), "classes" if "classes" in name else "P"
        said = lambda case: cases["order/%s/%s" % (name, case)]["error"]  # noqa: E731
        # the six checks, under the mismatch family's bounds and noun, in their order ...
        checks = [("pat_null", "%s is NULL" % what), ("m_over", "pattern length 65 outside [1,64]"), ("k_over", "k = 8 mismatches, at most 7"),
                  ("text_null", "text handle is NULL"), ("n_beyond", "range [10,+91) outside the text (100 bytes)"), ("count_null", "count must not be NULL")]
        assert said("m_zero") == name + ": pattern length 0 outside [1,64]"
        for i, (first, says) in enumerate(checks):
            assert said(first) == name + ": " + says
            for second, _ in checks[i + 1:]:
                assert said(first + "+" + second) == name + ": " + says, (name, first, second)
        # ... in the finds behind `positions NULL with cap > 0`, which comes before everything ...
        if find:
            assert said("out_null") == name + ": positions NULL with cap > 0"
            for second, _ in checks:
                assert said("out_null+" + second) == said("out_null"), (name, second)
        else:
            assert "order/%s/out_null" % name not in cases
        assert all(v["rc"] == -3 and v["device"] == 0 and v["written"] == "-" for c, v in cases.items() if c.startswith("order/%s/" % name))
        # ... and all of them before the refusal of a kernel that is not linked, which comes before the device
        missing, device = cases["missing/" + name], cases["device/" + name]
        assert (missing["rc"], missing["device"]) == (-4, 0)
        assert missing["error"] == "%s: this program holds no text_mis_%s kernel (k_tmis.hip is not linked)" % (name, "find" if find else "scan")
        assert (device["rc"], device["device"], device["launchers"], device["written"]) == (-4, 1, 0, "-")


def test_the_python_classes_calls_refuse_another_shape():
    for bad in (np.zeros(32, dtype=np.uint8), np.zeros((4, 31), dtype=np.uint8), np.zeros((2, 2, 32), dtype=np.uint8)):
        with pytest.raises(ValueError, match=r"\(m, 32\)"):
            engine.search_mis_classes(bad, None, 1, n=0)
        with pytest.raises(ValueError, match=r"\(m, 32\)"):
            engine.find_mis_classes(bad, None, 1, n=0)


# ---- the masks and the lanes' walk on the CPU --------------------------------------------------------------------------

def test_masks_and_walk_on_the_host(tmp_path):
    """tests/text_mis_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process: mis_neq_bytes /
    mis_neq_classes bit by bit (bytes 0 and 255, a repeated byte, empty and full rows, zero from m on; m = 1, 2, 31, 32, 33,
    63, 64); and every lane walking its run from a fresh start m - 1 bytes before it (edit_run_walk, mis_step, mis_hit,
    mis_raw) against the definition's triple loop, for those seven lengths and every k = 0 .. 7, on a text of three runs
    with planted copies at 0, k - 1, k and k + 1 substitutions, the range cut by e_begin, by e_end and by both at EVERY
    offset of the text."""
    exe = tmp_path / "text_mis_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "text_mis_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # the masks: 7 lengths x 3 checks; the walk: 7 lengths x 8 budgets (each over every cut of the text)
    assert r.returncode == 0 and failures == 0 and cases == 7 * 3 + 7 * 8, r.stdout[-4000:] + r.stderr[-2000:]


# ---- the compiled kernels --------------------------------------------------------------------------------------------------

def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """text_mis_scan and text_mis_find, for every (WORDS, BITS), are kernels of the k_tmis code object, each with ScratchSize 0
    and no static LDS (-Rpass-analysis=kernel-resource-usage, as tests/test_text_edit.py reads it)."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_tmis.hip")]
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
            for bits in (1, 2, 3):
                mine = [k for k in usage if re.search(r"text_mis_%sILi%dELi%dEE" % (kind, words, bits), k)]
                assert len(mine) == 1, (kind, words, bits, sorted(usage))
                assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
