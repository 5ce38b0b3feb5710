"""Mismatches on packed texts (smartgpu_psearch_mis64, smartgpu_pfind_mis64) without a GPU: the declarations, the bindings of
both libraries, the source registry, the documentation, the refusals that are decided before the first HIP call, and the
compiled kernels planes_mis_scan / planes_mis_find."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_psearch_mis64": 9, "smartgpu_pfind_mis64": 10}
ERR_ARG = -3


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def test_header_declares_both_calls_and_the_bound():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    assert re.search(r"^#define\s+SMARTGPU_PMIS_MAX\s+7\b", text, flags=re.M)


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
    for name in ("psearch_mis", "pfind_mis"):
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_names_both_kernels():
    for k in ("planes_mis_scan", "planes_mis_find"):
        assert sources.KERNEL_UNIT[k] == "k_planes"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_planes") == sources.kernel_sha256("planes_scan")


def test_integration_md_names_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + ["psearch_mis", "pfind_mis", "SMARTGPU_PMIS_MAX"]:
        assert n in doc, n


def _refused(rc, says):
    """-3 and a message that names the reason (`says`), so that each case is refused for what its comment states."""
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


def test_refusals_that_need_no_device():
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call.
    (A range outside a REAL text is refused in tests/test_packed_mis_gpu.py; here the NULL handle is what the range case meets.)"""
    L = engine.lib()
    P = np.full(4201, 65, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    mis = np.zeros(8, dtype=np.uint8)
    c = ctypes.c_uint64(77)
    pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    times = (ctypes.byref(pre), ctypes.byref(run))
    _refused(L.smartgpu_psearch_mis64(None, 4, 1, None, 0, 100, ctypes.byref(c), *times), "P is NULL")
    _refused(L.smartgpu_psearch_mis64(P.ctypes.data, 0, 1, None, 0, 100, ctypes.byref(c), *times), "length 0 ")
    _refused(L.smartgpu_psearch_mis64(P.ctypes.data, 4201, 1, None, 0, 5000, ctypes.byref(c), *times), "length 4201 ")  # m > SMARTGPU_XSIZE
    _refused(L.smartgpu_psearch_mis64(P.ctypes.data, 4, 8, None, 0, 100, ctypes.byref(c), *times), "k = 8 ")         # k > SMARTGPU_PMIS_MAX
    _refused(L.smartgpu_psearch_mis64(P.ctypes.data, 4, 1, None, 0, 100, ctypes.byref(c), *times), "handle is NULL")
    _refused(L.smartgpu_psearch_mis64(P.ctypes.data, 4, 1, None, 1 << 40, 100, ctypes.byref(c), *times), "handle is NULL")  # a range outside the text
    _refused(L.smartgpu_psearch_mis64(P.ctypes.data, 4, 1, None, 0, 100, None, *times), "handle is NULL")             # and count == NULL
    assert c.value == 77 and pre.value == -1.0 and run.value == -2.0  # a refused call writes nothing
    find = lambda p, m, k, off, n, pos, cap, cnt: L.smartgpu_pfind_mis64(p, m, k, None, off, n, pos, mis.ctypes.data, cap, cnt)  # noqa: E731
    _refused(find(None, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "P is NULL")
    _refused(find(P.ctypes.data, 0, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "length 0 ")
    _refused(find(P.ctypes.data, 4201, 1, 0, 5000, out.ctypes.data, 8, ctypes.byref(c)), "length 4201 ")
    _refused(find(P.ctypes.data, 4, 8, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "k = 8 ")
    _refused(find(P.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 1 << 40, 100, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, None), "handle is NULL")                           # and count == NULL
    _refused(find(P.ctypes.data, 4, 1, 0, 100, None, 8, ctypes.byref(c)), "positions NULL")                           # positions == NULL, cap > 0
    assert c.value == 77 and not out.any() and not mis.any()


def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """planes_mis_scan and planes_mis_find, for one and two planes and counters of 1, 2 and 3 bits, are kernels of the
    k_planes code object, each with ScratchSize 0 and no static LDS (-Rpass-analysis=kernel-resource-usage, as
    tests/test_packed_sets.py reads it)."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_planes.hip")]
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
            for bits in (1, 2, 3):
                mine = [k for k in usage if re.search(r"planes_mis_%sILi%dELi%dEE" % (kind, planes, bits), k)]
                assert len(mine) == 1, (kind, planes, bits, sorted(usage))
                assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
