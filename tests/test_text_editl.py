"""Edit distance for long patterns on byte texts (smartgpu_search_editl64, smartgpu_find_editl64 and their classes forms)
without a GPU: the declarations and bindings of both libraries, the source registry, the documents, the refusals that are
decided before the first HIP call, the masks, the geometry and the kernels' walk on the CPU under sanitizers
(tests/text_editl_check.cpp), and the compiled kernels.  The oracle of the GPU tests is tests/test_packed_edit.py's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_search_editl64": 10, "smartgpu_find_editl64": 11, "smartgpu_search_editl_classes64": 10, "smartgpu_find_editl_classes64": 11}
CONSTANTS = {"SMARTGPU_EDITL_MAXM": "256", "SMARTGPU_EDITL_MAXK": "31", "SMARTGPU_EDITL_ALL_BLOCKS": "1u"}
PYTHON = ("search_editl", "find_editl", "search_editl_classes", "find_editl_classes")
ERR_ARG = -3


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


# ---- declarations, bindings, registry, documents -----------------------------------------------------------------------

def test_header_declares_the_calls_and_the_constants():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define\s+%s\s+%s\s*$" % (name, value), text, flags=re.M), name
    assert re.search(r"^#define\s+SMARTGPU_EDIT_MAXM\s+64\b", text, flags=re.M)  # the existing calls keep their bound


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
    assert sources.UNITS["k_teditl"] == ("k_teditl.hip", "teditl.hpp", "teditl_host.hpp", "edit_block.hpp", "planes.hpp")
    for f in sources.UNITS["k_teditl"]:
        assert os.path.exists(os.path.join(sources.CSRC, f)), f
    for k in ("text_editl_scan", "text_editl_find"):
        assert sources.KERNEL_UNIT[k] == "k_teditl"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_teditl") != sources.unit_sha256("k_tedit")
    assert sources.UNITS["k_tedit"] == ("k_tedit.hip", "text_tile.hpp", "tedit.hpp", "tedit_host.hpp", "edit_step.hpp", "planes.hpp")
    assert sources.UNITS["k_tmis"] == ("k_tmis.hip", "text_tile.hpp", "tmis.hpp", "tmis_host.hpp", "tedit_host.hpp", "edit_step.hpp", "planes.hpp")
    assert sources.UNITS["k_talign"] == ("k_talign.hip", "talign.hpp", "talign_host.hpp", "tedit.hpp", "tedit_host.hpp", "edit_align.hpp", "edit_step.hpp",
                                         "planes.hpp")
    assert sources.UNITS["k_peditl"] == ("k_peditl.hip", "peditl.hpp", "peditl_host.hpp", "edit_block.hpp", "planes.hpp")
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_teditl\b", makefile, flags=re.M)
    for h in ("teditl.hpp", "teditl_host.hpp", "edit_block.hpp"):
        assert re.search(r"^HEADERS\s*:=.*\b%s\b" % re.escape(h), makefile, flags=re.M), h


def test_the_host_header_is_host_only():
    """teditl_host.hpp: no HIP call, no error text, and the block recurrence's header."""
    text = open(os.path.join(sources.CSRC, "teditl_host.hpp")).read()
    code = re.sub(r"//.*", "", text)
    assert '#include "edit_block.hpp"' in code
    assert "hip" not in code.replace("__HIPCC__", "") and "set_error" not in code and "printf" not in code


def test_documents_name_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + list(PYTHON) + list(CONSTANTS):
        assert n in doc, n
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "smartgpu_search_editl64" in readme and "smartgpu_find_editl64" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "text_editl_scan" in design and "text_editl_find" in design and "k_teditl.hip" in design
    header = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    assert "ALIGNMENTS of long patterns on a byte text" in header  # NOT offered, and said so
    assert "NOT offered: m > 64 and k > 7 (smartgpu_search_editl64" in header  # the short calls point here
    assert "tools/teditl_probe.py" in header and os.path.exists(os.path.join(ROOT, "tools", "teditl_probe.py"))


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_classes"])
def test_refusals_that_need_no_device(kind):
    """Every call passes a NULL text, so each is decided before the first HIP call, and a refused call writes nothing."""
    L = engine.lib()
    what = "classes is NULL" if kind else "P is NULL"
    name = "search_editl%s64" % kind
    P = np.full(300 * 32, 1, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    dist = np.zeros(8, dtype=np.uint8)
    c = ctypes.c_uint64(77)
    pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    times = (ctypes.byref(pre), ctypes.byref(run))
    count = getattr(L, "smartgpu_search_editl%s64" % kind)
    _refused(count(None, 4, 1, 0, None, 0, 100, ctypes.byref(c), *times), name + ": " + what)
    _refused(count(P.ctypes.data, 0, 1, 0, None, 0, 100, ctypes.byref(c), *times), "pattern length 0 outside [1,256]")
    _refused(count(P.ctypes.data, 257, 1, 0, None, 0, 1000, ctypes.byref(c), *times), "pattern length 257 outside [1,256]")
    _refused(count(P.ctypes.data, 4, 32, 0, None, 0, 100, ctypes.byref(c), *times), "k = 32 edits, at most 31")
    _refused(count(P.ctypes.data, 4, 1, 2, None, 0, 100, ctypes.byref(c), *times), "flags 0x2")
    _refused(count(P.ctypes.data, 4, 1, 3, None, 0, 100, ctypes.byref(c), *times), "flags 0x3")
    _refused(count(P.ctypes.data, 256, 31, 1, None, 0, 100, ctypes.byref(c), *times), name + ": text handle is NULL")  # all legal but the handle
    _refused(count(P.ctypes.data, 65, 8, 0, None, 1 << 40, 100, ctypes.byref(c), *times), "handle is NULL")           # a range outside the text
    _refused(count(P.ctypes.data, 4, 1, 0, None, 0, 100, None, *times), "handle is NULL")                             # and count == NULL
    assert c.value == 77 and pre.value == -1.0 and run.value == -2.0
    f = getattr(L, "smartgpu_find_editl%s64" % kind)
    find = lambda p, m, k, fl, pos, cap, cnt: f(p, m, k, fl, None, 0, 1000, pos, dist.ctypes.data, cap, cnt)  # noqa: E731
    _refused(find(None, 4, 1, 0, out.ctypes.data, 8, ctypes.byref(c)), what)
    _refused(find(P.ctypes.data, 0, 1, 0, out.ctypes.data, 8, ctypes.byref(c)), "pattern length 0 outside [1,256]")
    _refused(find(P.ctypes.data, 257, 1, 0, out.ctypes.data, 8, ctypes.byref(c)), "pattern length 257 outside [1,256]")
    _refused(find(P.ctypes.data, 4, 32, 0, out.ctypes.data, 8, ctypes.byref(c)), "k = 32 edits, at most 31")
    _refused(find(P.ctypes.data, 4, 1, 2, out.ctypes.data, 8, ctypes.byref(c)), "flags 0x2")
    _refused(find(P.ctypes.data, 4, 1, 3, out.ctypes.data, 8, ctypes.byref(c)), "flags 0x3")
    _refused(find(P.ctypes.data, 256, 31, 1, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 0, out.ctypes.data, 8, None), "handle is NULL")                        # and count == NULL
    _refused(find(P.ctypes.data, 4, 1, 0, None, 8, ctypes.byref(c)), "ends NULL with cap > 0")                # ends == NULL, cap > 0
    assert c.value == 77 and not out.any() and not dist.any()


def test_the_short_calls_keep_their_bounds_and_messages():
    """New symbols only: smartgpu_search_edit64 still stops at 64 bytes and 7 edits, in the same words."""
    L = engine.lib()
    P = np.full(300, 1, dtype=np.uint8)
    c = ctypes.c_uint64(77)
    _refused(L.smartgpu_search_edit64(P.ctypes.data, 65, 1, None, 0, 100, ctypes.byref(c), None, None), "length 65 outside [1,64]")
    _refused(L.smartgpu_search_edit64(P.ctypes.data, 4, 8, None, 0, 100, ctypes.byref(c), None, None), "k = 8 edits, at most 7")
    assert c.value == 77


def test_the_python_classes_calls_refuse_another_shape():
    for bad in (np.zeros(32, dtype=np.uint8), np.zeros((4, 31), dtype=np.uint8)):
        with pytest.raises(ValueError, match=r"\(m, 32\)"):
            engine.search_editl_classes(bad, None, 1)
        with pytest.raises(ValueError, match=r"\(m, 32\)"):
            engine.find_editl_classes(bad, None, 1)


# ---- the masks, the geometry and the walk on the CPU ---------------------------------------------------------------------

def test_masks_geometry_and_the_kernels_walk_on_the_host(tmp_path):
    """tests/text_editl_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process (no library is preloaded
    anywhere).  editl_peq_bytes / editl_peq_classes bit by bit and editl_peq_table's word-major order; editl_run_walk,
    editl_tile_count and editl_first_piece against restatements; and the walk of k_teditl.hip as the kernels run it — super-tiles,
    trips from j0 = -ceil((m + k) / piece), 64 lanes in step with one number of active blocks, starts clipped at e_begin, neutral
    votes of the lanes outside the range — against a scalar DP on the range, every end position reported exactly once with its
    distance: m = 1, 32, 33, 64, 65, 96, 97, 128, 129, 255, 256; k = 0, 1, 7, 8, 15, 16, 31; alphabets of 2, 4, 20 and 256 values;
    byte patterns (with copies planted at the seams of runs, waves and super-tiles) and class patterns; with the cut-off and
    with all blocks; texts of one to three super-tiles' worth of runs on a grid scaled down to runs of 128 in pieces of 32, and
    two cases on the product's own 512 / 128 / 256.  Per length, for k = 0, 7, 31, a text of planted prefixes (31, 32, 33, 64,
    100, 200, m - 1 bytes, each followed by a byte that is not accepted), where the program itself asserts that the second
    block was switched on and, for k <= 7, that a block was switched off again."""
    exe = tmp_path / "text_editl_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "text_editl_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # the masks: 4 alphabets x 4 lengths x 3 checks; the geometry: 5; per length 4 alphabets x 2 kinds of pattern x 7 budgets x
    # (cut-off, all blocks) + 3 budgets of planted prefixes, 11 lengths; the product's geometry: 2
    assert r.returncode == 0 and failures == 0 and cases == 4 * 4 * 3 + 5 + 11 * (4 * 2 * 7 * 2 + 3) + 2, r.stdout[-4000:] + r.stderr[-2000:]


def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """text_editl_scan and text_editl_find for 2, 4 and 8 dwords are kernels of the k_teditl code object, each exactly once,
    with ScratchSize 0 (pv / mv are indexed by constants only) and no static LDS: flush_hits' bytes, the masks and the rows
    are dynamic."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_teditl.hip")]
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
        for words in (2, 4, 8):
            mine = [k for k in usage if re.search(r"text_editl_%sILi%dEE" % (kind, words), k)]
            assert len(mine) == 1, (kind, words, sorted(usage))
            assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
    assert len([k for k in usage if "text_editl_" in k]) == 6, sorted(usage)
