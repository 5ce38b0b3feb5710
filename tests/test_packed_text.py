"""Packed texts (smartgpu_ptext, bit planes) without a GPU: the layout arithmetic, the bindings of both libraries,
the source registry of the new kernel unit, and the documentation of every new declaration."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def declared_ptext_symbols():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(smartgpu_p(?:text_[a-z0-9_]+|search[a-z0-9_]*))\s*\(", text)))


EXPECTED = ["smartgpu_psearch64", "smartgpu_psearch_batch64", "smartgpu_ptext_bytes", "smartgpu_ptext_device", "smartgpu_ptext_free",
            "smartgpu_ptext_layout", "smartgpu_ptext_length", "smartgpu_ptext_pack", "smartgpu_ptext_planes", "smartgpu_ptext_read",
            "smartgpu_ptext_symbols", "smartgpu_ptext_upload"]


def test_header_declares_the_packed_text_abi():
    names = declared_ptext_symbols()
    for n in EXPECTED:
        assert n in names, n


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 2**32, 2**35 + 5])
def test_layout(n):
    for k in (1, 2, 3, 4):
        planes, nbytes = smart_amd.ptext_layout(n, k)
        assert planes == (1 if k <= 2 else 2), (n, k)
        assert nbytes == 4 * ((n + 31) // 32), (n, k)


@pytest.mark.parametrize("k", [-1, 0, 5, 256])
def test_layout_refuses_other_value_counts(k):
    L = engine.lib()
    planes, nbytes = ctypes.c_int(0), ctypes.c_uint64(0)
    assert L.smartgpu_ptext_layout(100, k, ctypes.byref(planes), ctypes.byref(nbytes)) == -3  # SMARTGPU_ERR_ARG
    assert str(k) in L.smartgpu_last_error().decode()
    with pytest.raises(smart_amd.SmartGpuError):
        smart_amd.ptext_layout(100, k)


def test_layout_accepts_null_outputs():
    assert engine.lib().smartgpu_ptext_layout(100, 4, None, None) == 0


def test_both_libraries_bind_every_new_symbol():
    for path in (engine.LIB_PATH, engine.AB_LIB_PATH):
        L = engine._load(path)
        for n in declared_ptext_symbols():
            f = getattr(L, n)
            assert f.argtypes is not None, (path, n)  # the engine gave it a prototype
    for name in ("PackedText", "psearch", "psearch_batch", "ptext_layout"):
        assert hasattr(smart_amd, name), name
    for attr in ("pack", "upload", "read", "planes", "nbytes", "symbols", "free", "__len__", "__enter__", "__exit__"):
        assert hasattr(smart_amd.PackedText, attr), attr


def test_sources_registry_has_the_planes_unit():
    assert "k_planes" in sources.UNITS
    own = [f for f in sources.UNITS["k_planes"] if f.startswith("k_")]
    assert own == ["k_planes.hip"]
    assert "planes.hpp" in sources.UNITS["k_planes"]
    for p in sources.unit_files("k_planes"):
        assert os.path.exists(p), p
    assert sources.KERNEL_UNIT["planes_scan"] == "k_planes" and sources.KERNEL_UNIT["planes_pack"] == "k_planes"
    shas = sources.all_unit_shas()
    mine = sources.kernel_sha256("planes_scan")
    assert mine == shas["k_planes"]
    assert all(mine != s for u, s in shas.items() if u != "k_planes")
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_planes\b", makefile, flags=re.M)


def test_new_declarations_are_documented_in_integration_md():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in declared_ptext_symbols():
        assert n in doc, n
