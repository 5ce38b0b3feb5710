"""Starts and alignments of LONG edit-distance occurrences on packed texts (smartgpu_palign_editl64,
smartgpu_palign_sets_editl64: m <= 256, k <= 31) without a GPU: the declarations and bindings of both libraries, where the
exported functions and their one host path live, the source registry, the documents, the refusals that are decided before
the first HIP call, the band of alignl_band.hpp fed from a plane window on the CPU under sanitizers
(tests/packed_alignl_check.cpp), and the compiled kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_palign_editl64": 11, "smartgpu_palign_sets_editl64": 11}
PYTHON = ("palign_editl", "palign_sets_editl", "pfind_editl_align", "pfind_sets_editl_align")
ERR_ARG = -3
WORDS = 10  # SMARTGPU_ALIGNL_OPS_WORDS


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
    # the long find and the short align call point at the new calls, and no longer say there is nothing
    assert "ALIGNMENTS of long patterns on a packed text: smartgpu_palign_editl64 below" in raw
    assert "smartgpu_palign_edit64 stays at m <=" not in raw and "their alignments are not offered" not in raw
    assert "k_palignl.hip" in raw and "tools/palignl_probe.py" in raw and "planes_editl_align" in raw


def test_both_libraries_export_and_bind_them():
    for path in (engine.LIB_PATH, engine.AB_LIB_PATH):
        raw = ctypes.CDLL(path)
        L = engine._load(path)
        for n, nargs in SYMBOLS.items():
            assert hasattr(raw, n), (path, n)
            f = getattr(L, n)
            assert f.argtypes is not None and f.restype is ctypes.c_int, (path, n)
            assert len(f.argtypes) == nargs, (path, n)
        # the host path the two wrappers share has C++ linkage and is no dynamic symbol
        dyn = subprocess.run(["nm", "-D", "--defined-only", "-C", path], capture_output=True, text=True, check=True).stdout
        assert "palignl_run" not in dyn, path


def test_python_functions_exist():
    for name in PYTHON:
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_has_the_unit_and_the_calls_live_in_their_own_host_unit():
    assert [f for f in sources.UNITS["k_palignl"] if f.startswith("k_")] == ["k_palignl.hip"]
    for f in ("palignl.hpp", "alignl_band.hpp", "talign_host.hpp", "peditl_host.hpp", "edit_align.hpp", "planes.hpp"):
        assert f in sources.UNITS["k_palignl"], f
        assert os.path.exists(os.path.join(sources.CSRC, f)), f
    assert sources.KERNEL_UNIT["planes_editl_align"] == "k_palignl"
    sha = sources.unit_sha256("k_palignl")
    assert sources.kernel_sha256("planes_editl_align") == sha and sha not in (sources.unit_sha256("k_palign"), sources.unit_sha256("k_talignl"))
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_palignl\b", makefile, flags=re.M)
    assert re.search(r"^UNITS\s*:=.*\bpalignl_calls\b", makefile, flags=re.M)
    assert re.search(r"^HEADERS\s*:=.*\$\(HERE\)palignl\.hpp\b", makefile, flags=re.M)
    variant = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    assert re.search(r"\bk_palignl\b", variant) and re.search(r"\bpalignl_calls\b", variant)
    # the two exported functions are one-line wrappers in their own unit; the family and the host path are align_calls.cpp's
    unit = open(os.path.join(sources.CSRC, "palignl_calls.cpp")).read()
    assert set(re.findall(r"^int smartgpu_([a-z0-9_]+)\(", unit, flags=re.M)) == {"palign_editl64", "palign_sets_editl64"}
    assert unit.count("return palignl_run(") == 2
    calls = open(os.path.join(sources.CSRC, "align_calls.cpp")).read()
    assert "struct PAlignl : PQuestion" in calls and "return align_run<PAlignl>(" in calls and "g_planes_editl_align" in calls
    assert not re.search(r"^int smartgpu_palign(_sets)?_editl64\(", calls, flags=re.M)
    # the kernel takes everything a lane decides by itself from alignl_band.hpp
    kernel = open(os.path.join(sources.CSRC, "k_palignl.hip")).read()
    for helper in ("alignl_step_cell", "alignl_cell", "alignl_miss", "alignl_dec_shift", "alignl_dec_flush", "alignl_dec_dword", "alignl_dec_lane",
                   "alignl_key", "alignl_key_dist", "alignl_key_j", "alignl_walk_step", "alignl_op_word", "alignl_op_bits"):
        assert re.search(r"\b%s\(" % helper, kernel), helper


def test_documents_name_every_symbol():
    names = list(SYMBOLS) + list(PYTHON) + ["planes_editl_align", "k_palignl.hip"]
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for n in names:
            assert n in text, (doc, n)
    results = open(os.path.join(ROOT, "profiles", "packed", "RESULTS.md")).read()
    assert "Long patterns: starts and alignments" in results and "palignl_probe.py" in results
    assert os.path.exists(os.path.join(ROOT, "tools", "palignl_probe.py"))


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_sets"])
def test_refusals_that_need_no_device(kind):
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call, for
    the reason its line states, in smartgpu_palign_edit64's order, and writes nothing.  (An end outside a REAL range, a set
    that names a code the text does not hold and a three-plane text are refused in tests/test_packed_alignl_gpu.py.)"""
    f = getattr(engine.lib(), "smartgpu_palign%s_editl64" % kind)
    P = np.full(300, 1, dtype=np.uint8)
    ends = np.arange(8, dtype=np.uint64)
    starts = np.full(8, 77, dtype=np.uint64)
    dist = np.full(8, 7, dtype=np.uint8)
    ops = np.full(8 * WORDS, 5, dtype=np.uint64)
    call = lambda p, m, k, e, cnt, s: f(p, m, k, None, 0, 1000, e, cnt, s, dist.ctypes.data, ops.ctypes.data)  # noqa: E731
    _refused(call(None, 100, 9, ends.ctypes.data, 8, starts.ctypes.data), "sets is NULL" if kind else "P is NULL")
    _refused(call(P.ctypes.data, 0, 9, ends.ctypes.data, 8, starts.ctypes.data), "length 0 outside [1,256]")
    _refused(call(P.ctypes.data, 257, 9, ends.ctypes.data, 8, starts.ctypes.data), "length 257 outside [1,256]")
    _refused(call(P.ctypes.data, 100, 32, ends.ctypes.data, 8, starts.ctypes.data), "k = 32 edits, at most 31")
    assert ("palign%s_editl64:" % kind) in engine.lib().smartgpu_last_error().decode()
    _refused(call(P.ctypes.data, 100, 9, None, 8, starts.ctypes.data), "ends NULL with count > 0")
    _refused(call(P.ctypes.data, 100, 9, ends.ctypes.data, 8, None), "starts NULL with count > 0")
    assert ("palign%s_editl64:" % kind) in engine.lib().smartgpu_last_error().decode()
    _refused(call(P.ctypes.data, 100, 9, ends.ctypes.data, 8, starts.ctypes.data), "packed text handle is NULL")
    _refused(call(P.ctypes.data, 256, 31, ends.ctypes.data, 8, starts.ctypes.data), "packed text handle is NULL")  # the largest legal m and k pass the bounds
    _refused(call(P.ctypes.data, 100, 9, None, 0, None), "packed text handle is NULL")  # count == 0 excuses the NULL lists, not the NULL text
    # the order: a missing list before the pattern's checks, the pattern before its length, the length before k, k before the handle
    _refused(call(None, 0, 32, None, 8, starts.ctypes.data), "ends NULL with count > 0")
    _refused(call(None, 0, 32, ends.ctypes.data, 8, None), "starts NULL with count > 0")
    _refused(call(None, 0, 32, ends.ctypes.data, 8, starts.ctypes.data), "is NULL")
    _refused(call(P.ctypes.data, 0, 32, ends.ctypes.data, 8, starts.ctypes.data), "length 0 outside [1,256]")
    _refused(call(P.ctypes.data, 257, 32, ends.ctypes.data, 8, starts.ctypes.data), "length 257 outside [1,256]")
    _refused(call(P.ctypes.data, 256, 32, ends.ctypes.data, 8, starts.ctypes.data), "k = 32 edits, at most 31")
    # and the short call's lines for the same violations differ only in the name and the bounds
    g = getattr(engine.lib(), "smartgpu_palign%s_edit64" % kind)
    short_ops = np.full(8 * 3, 5, dtype=np.uint64)
    for args, says in (((None, 20, 3, ends.ctypes.data, 8, starts.ctypes.data), "is NULL"), ((P.ctypes.data, 20, 3, None, 8, starts.ctypes.data), "ends NULL"),
                       ((P.ctypes.data, 20, 3, ends.ctypes.data, 8, None), "starts NULL"), ((P.ctypes.data, 20, 3, ends.ctypes.data, 8, starts.ctypes.data), "handle is NULL")):
        p, m, k, e, cnt, s = args
        _refused(g(p, m, k, None, 0, 1000, e, cnt, s, dist.ctypes.data, short_ops.ctypes.data), says)
        short = engine.lib().smartgpu_last_error().decode()
        _refused(call(p, m, k, e, cnt, s), says)
        assert engine.lib().smartgpu_last_error().decode() == short.replace("_edit64:", "_editl64:"), short
    assert (starts == 77).all() and (dist == 7).all() and (ops == 5).all() and (ends == np.arange(8)).all()


# ---- the band on the CPU ---------------------------------------------------------------------------------------------------

def test_band_from_a_plane_window_on_the_host(tmp_path):
    """tests/packed_alignl_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process with no preload:
    alignl_band.hpp stepped lane by lane as the kernel steps it — the four masks of the reversed pattern (editl_peq_pattern /
    editl_peq_sets), codes from the 10-dword window of each plane with guard words around it, the packed decisions, the key
    reduction, the walk — against a scalar full-matrix DP written out in the program: start, distance, every operation and the
    packing.  m = 1, 31, 32, 33, 64, 65, 128, 129, 255, 256; k = 0, 1, 7, 8, 31; 1 to 4 values; bytes and sets; every e % 32;
    clipped ends with every number of columns from 1 to m + k; windows that begin below dword 0."""
    exe = tmp_path / "packed_alignl_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
           "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "packed_alignl_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # per length: 4 numbers of values x (bytes, sets) x 5 values of k, + (both kinds of end, every phase, clipped and small ends,
    # every number of columns seen); 10 lengths
    assert r.returncode == 0 and failures == 0 and cases == 10 * (4 * 2 * 5 + 1), r.stdout[-4000:] + r.stderr[-2000:]


def test_the_unit_holds_four_kernels_without_scratch_and_static_lds():
    """planes_editl_align for one and two planes, with and without the decisions: exactly four kernels of the k_palignl code
    object, each with ScratchSize 0 (-Rpass-analysis=kernel-resource-usage).  The LDS is static, so the compiler reports all
    of it: the masks (32 dwords) + four windows of 10 dwords per plane + (with ops) four waves x 17 x 64 dwords of decisions."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_palignl.hip")]
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
    assert len([k for k in usage if "planes_editl_align" in k]) == 4, sorted(usage)
    text = open(os.path.join(sources.CSRC, "k_palignl.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(\(planes_editl_align<p_, o_>\), dim3\(grid\), dim3\(kPAlignlT\), 0, stream, a\);", text)  # no dynamic LDS
    assert text.count("__syncthreads()") == 2 and text.index("__syncthreads();") < text.index("for (uint64_t idx")  # one barrier (and its mention), before the loop
    for planes in (1, 2):
        for ops in (0, 1):
            mine = [k for k in usage if re.search(r"planes_editl_alignILi%dELb%dEE" % (planes, ops), k)]
            assert len(mine) == 1, (planes, ops, sorted(usage))
            lds = 4 * (32 + 4 * 10 * planes + (4 * 17 * 64 if ops else 0))
            assert lds <= 65536
            assert usage[mine[0]] == {"scratch": 0, "lds": lds}, (mine[0], usage[mine[0]], lds)
