"""Positions on packed texts (smartgpu_pfind64, smartgpu_pfind_batch64) without a GPU: the declarations, the bindings of both
libraries, the source registry, the documentation, the refusals that are decided before the first HIP call, and the compiled
kernels planes_find<1> / planes_find<2>."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = ["smartgpu_pfind64", "smartgpu_pfind_batch64"]
ERR_ARG = -3


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def test_header_declares_both_calls():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n


def test_both_libraries_export_and_bind_them():
    for path in (engine.LIB_PATH, engine.AB_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), SYMBOLS[0]) and hasattr(ctypes.CDLL(path), SYMBOLS[1]), path
        L = engine._load(path)
        for n in SYMBOLS:
            f = getattr(L, n)
            assert f.argtypes is not None and f.restype is ctypes.c_int, (path, n)  # the engine gave it a prototype
    assert len(engine.lib().smartgpu_pfind64.argtypes) == 8
    assert len(engine.lib().smartgpu_pfind_batch64.argtypes) == 9


def test_python_functions_exist():
    for name in ("pfind", "pfind_batch"):
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_names_the_kernel():
    assert sources.KERNEL_UNIT["planes_find"] == "k_planes"
    assert sources.kernel_sha256("planes_find") == sources.kernel_sha256("planes_scan")


def test_the_wave_reservation_stands_once():
    """The find kernels' slots come from dev_common.hpp's wave_reserve: no unit keeps a prefix sum of its own
    (kernels_ab.inc holds the superseded kernels as they were)."""
    own = [os.path.basename(p) for p in glob.glob(os.path.join(sources.CSRC, "*.hip")) + glob.glob(os.path.join(sources.CSRC, "*.hpp"))
           if "__shfl_up(" in open(p).read()]
    assert own == ["dev_common.hpp"]


def test_integration_md_names_both_symbols():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in SYMBOLS + ["pfind_batch", "smart_amd.pfind"]:
        assert n in doc, n


def _refused(rc):
    assert rc == ERR_ARG, rc
    assert engine.lib().smartgpu_last_error().decode() != ""


def test_refusals_that_need_no_device():
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call."""
    L = engine.lib()
    P = np.full(4201, 65, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    c = ctypes.c_uint64(77)
    _refused(L.smartgpu_pfind64(P.ctypes.data, 4, None, 0, 100, out.ctypes.data, 8, ctypes.byref(c)))      # NULL text handle
    _refused(L.smartgpu_pfind64(P.ctypes.data, 0, None, 0, 100, out.ctypes.data, 8, ctypes.byref(c)))      # m = 0
    _refused(L.smartgpu_pfind64(P.ctypes.data, 4201, None, 0, 5000, out.ctypes.data, 8, ctypes.byref(c)))  # m = 4201
    _refused(L.smartgpu_pfind64(P.ctypes.data, 4, None, 0, 100, out.ctypes.data, 8, None))                 # count == NULL
    _refused(L.smartgpu_pfind64(P.ctypes.data, 4, None, 0, 100, None, 8, ctypes.byref(c)))                 # positions == NULL, cap > 0
    assert c.value == 77 and not out.any()  # a refused call writes nothing
    ptrs = (ctypes.c_void_p * 2)(P.ctypes.data, P.ctypes.data)
    set_ = ctypes.cast(ptrs, ctypes.c_void_p)
    starts = np.zeros(3, dtype=np.uint64)
    _refused(L.smartgpu_pfind_batch64(set_, 4, 0, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data))   # K = 0
    _refused(L.smartgpu_pfind_batch64(set_, 4, 2, None, 0, 100, out.ctypes.data, 8, None))                 # starts == NULL
    _refused(L.smartgpu_pfind_batch64(set_, 4, 2, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data))   # NULL text handle
    _refused(L.smartgpu_pfind_batch64(set_, 0, 2, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data))   # m = 0
    _refused(L.smartgpu_pfind_batch64(set_, 4201, 2, None, 0, 5000, out.ctypes.data, 8, starts.ctypes.data))
    _refused(L.smartgpu_pfind_batch64(None, 4, 2, None, 0, 100, out.ctypes.data, 8, starts.ctypes.data))   # P == NULL


def test_the_unit_holds_both_kernels_and_only_vector_stores(tmp_path):
    """planes_find<1> and planes_find<2> are kernels of the k_planes code object, without scratch and static LDS, and
    every instruction of the scalar unit that touches memory in them is a load."""
    asm = str(tmp_path / "k_planes.s")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm,
           os.path.join(sources.CSRC, "k_planes.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    text = open(asm).read()
    for planes in (1, 2):
        name = "_ZN2sg11planes_findILi%dEEEvNS_9PlaneArgsEPyy" % planes
        assert re.search(r"^\s*\.amdhsa_kernel\s+%s\s*$" % name, text, flags=re.M), name
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index(".Lfunc_end")]
        desc = text[text.index(".amdhsa_kernel %s" % name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", desc), name
        assert re.search(r"\.amdhsa_group_segment_fixed_size\s+0\b", desc), name
        insts = [ln.split()[0] for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]
        scalar_mem = [i for i in insts if i.startswith("s_") and re.search(r"dword|scratch|buffer|store|atomic", i)]
        assert scalar_mem and all(re.fullmatch(r"s_(buffer_)?load_dword(x\d+)?", i) for i in scalar_mem), sorted(set(scalar_mem))
        assert "global_store_dwordx2" in insts, name       # the positions: 64-bit vector stores
        assert insts.count("global_atomic_add_x2") >= 1, name  # the cursor
