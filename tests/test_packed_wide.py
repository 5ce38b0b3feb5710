"""Packed texts of five to eight values on three bit planes (smartgpu_ptext_layout8, smartgpu_ptext_pack8,
smartgpu_ptext_upload8, smartgpu_ptext_symbols8, smartgpu_iupac_sets8) without a GPU: the declarations, the bindings of both
libraries, the Python names, the source registry, the layout arithmetic, the IUPAC table over a text with N, the refusals
that are decided before the first HIP call, and the documentation."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_ptext_layout8": 4, "smartgpu_ptext_pack8": 1, "smartgpu_ptext_upload8": 3, "smartgpu_ptext_symbols8": 2,
           "smartgpu_iupac_sets8": 5}
ERR_ARG = -3

# the bases every IUPAC nucleotide letter accepts
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
ACGNT = b"ACGNT"  # ascending: N is code 3, T code 4


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def test_header_declares_the_five_calls_and_the_macro():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    assert re.search(r"^#define SMARTGPU_PTEXT_MAXVALUES 8\b", text, flags=re.M)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n


def test_both_libraries_export_and_bind_them():
    for path in (engine.LIB_PATH, engine.AB_LIB_PATH):
        raw = ctypes.CDLL(path)
        L = engine._load(path)
        for n, nargs in SYMBOLS.items():
            assert hasattr(raw, n), (path, n)
            f = getattr(L, n)
            assert f.argtypes is not None and len(f.argtypes) == nargs, (path, n)  # the engine gave it a prototype
            assert f.restype is (ctypes.c_void_p if n in ("smartgpu_ptext_pack8", "smartgpu_ptext_upload8") else ctypes.c_int), (path, n)


def test_python_names_exist():
    assert smart_amd.ptext_layout8 is engine.ptext_layout8 and callable(smart_amd.ptext_layout8)
    import inspect
    assert "wide" in inspect.signature(smart_amd.PackedText.upload).parameters
    assert "wide" in inspect.signature(smart_amd.PackedText.pack).parameters
    assert inspect.signature(smart_amd.PackedText.upload).parameters["wide"].default is False
    assert inspect.signature(smart_amd.PackedText.pack).parameters["wide"].default is False


def test_sources_registry_names_the_unit_and_its_kernels():
    assert sources.UNITS["k_planes3"] == ("k_planes3.hip", "planes3.hpp", "planes3_host.hpp", "planes.hpp")
    assert sources.UNITS["k_planes"] == ("k_planes.hip", "planes.hpp")
    for k in ("planes3_pack", "planes3_scan", "planes3_find"):
        assert sources.KERNEL_UNIT[k] == "k_planes3"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_planes3")
    # the unit's own file is k_planes3.hip only: every other .hip belongs to another unit
    hips = [f for f in sources.UNITS["k_planes3"] if f.endswith(".hip")]
    assert hips == ["k_planes3.hip"]
    assert not [u for u, files in sources.UNITS.items() if u != "k_planes3" and "k_planes3.hip" in files]
    for f in sources.UNITS["k_planes3"]:
        assert os.path.exists(os.path.join(sources.CSRC, f)), f
    mk = open(os.path.join(sources.CSRC, "Makefile")).read()
    kernels = re.search(r"^KERNELS := (.*)$", mk, flags=re.M).group(1).split()
    headers = re.search(r"^HEADERS := (.*)$", mk, flags=re.M).group(1)
    assert "k_planes3" in kernels and "planes3.hpp" in headers and "planes3_host.hpp" in headers


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 2**32, 2**35 + 5])
def test_layout8(n):
    for nvalues in range(1, 9):
        planes, nbytes = smart_amd.ptext_layout8(n, nvalues)
        assert planes == (1 if nvalues <= 2 else 2 if nvalues <= 4 else 3), (n, nvalues)
        assert nbytes == 4 * ((n + 31) // 32), (n, nvalues)
        if nvalues <= 4:
            assert (planes, nbytes) == smart_amd.ptext_layout(n, nvalues)


def test_layout8_refusals_and_null_outputs():
    L = engine.lib()
    planes, nbytes = ctypes.c_int(77), ctypes.c_uint64(77)
    for bad in (0, 9, -1):
        assert L.smartgpu_ptext_layout8(100, bad, ctypes.byref(planes), ctypes.byref(nbytes)) == ERR_ARG
        assert str(bad) in L.smartgpu_last_error().decode()
        with pytest.raises(smart_amd.SmartGpuError):
            smart_amd.ptext_layout8(100, bad)
    assert planes.value == 77 and nbytes.value == 77  # a refused call writes nothing
    assert L.smartgpu_ptext_layout8(100, 5, None, None) == 0
    assert L.smartgpu_ptext_layout8(100, 5, ctypes.byref(planes), None) == 0 and planes.value == 3
    assert L.smartgpu_ptext_layout8(100, 8, None, ctypes.byref(nbytes)) == 0 and nbytes.value == 16
    # the four-value call still refuses what it refused
    assert L.smartgpu_ptext_layout(100, 5, ctypes.byref(planes), ctypes.byref(nbytes)) == ERR_ARG


def expected_sets(pattern, values):
    """The table written out: bit c of sets[j] = the base values[c] stands for is accepted by letter j; a value that is no
    base letter stands for none."""
    out = []
    for ch in pattern:
        bases = IUPAC[ch.upper()]
        s = 0
        for c, v in enumerate(values):
            base = {"U": "T"}.get(chr(v).upper(), chr(v).upper())
            if base in "ACGT" and base in bases:
                s |= 1 << c
        out.append(s)
    return out


def test_iupac8_all_letters_both_cases_over_acgnt():
    letters = "".join(IUPAC)
    for pattern in (letters, letters.lower()):
        got = smart_amd.iupac_sets(pattern.encode(), ACGNT, wide=True)
        assert got.dtype == np.uint8
        # A=1 C=2 G=4 T=16: code 3, the text's N, is in no set
        assert got.tolist() == [1, 2, 4, 16, 16, 5, 18, 6, 17, 20, 3, 22, 21, 19, 7, 23]
        assert got.tolist() == expected_sets(pattern, ACGNT)
        assert not (got & 8).any()  # N of the text is accepted by no letter, pattern N included
    assert smart_amd.iupac_sets("GGNCC", ACGNT, wide=True).tolist() == [4, 4, 23, 2, 2]
    assert smart_amd.iupac_sets(b"ACGU", b"ACGNU|", wide=True).tolist() == [1, 2, 4, 16]  # a separator is no base either
    assert smart_amd.iupac_sets(letters.encode(), b"acgnt", wide=True).tolist() == expected_sets(letters, ACGNT)
    eight = bytes([0, 1, 65, 67, 71, 78, 84, 255])
    assert smart_amd.iupac_sets(letters.encode(), eight, wide=True).tolist() == expected_sets(letters, eight)


def test_iupac8_with_four_values_is_iupac_sets():
    L = engine.lib()
    letters = np.frombuffer("".join(IUPAC).encode(), dtype=np.uint8).copy()
    for values in (b"ACGT", b"ACT", b"AT", b"G", b"ACGU"):
        vals = np.zeros(8, dtype=np.uint8)
        vals[:len(values)] = np.frombuffer(values, dtype=np.uint8)
        a, b = np.zeros(len(letters), dtype=np.uint8), np.zeros(len(letters), dtype=np.uint8)
        assert L.smartgpu_iupac_sets(vals.ctypes.data, len(values), letters.ctypes.data, len(letters), a.ctypes.data) == 0
        assert L.smartgpu_iupac_sets8(vals.ctypes.data, len(values), letters.ctypes.data, len(letters), b.ctypes.data) == 0
        assert a.tolist() == b.tolist() == expected_sets("".join(IUPAC), values), values
    # and the Python call without `wide` is the four-value call, refusals included
    assert smart_amd.iupac_sets(b"GGNCC", b"ACGT").tolist() == smart_amd.iupac_sets(b"GGNCC", b"ACGT", wide=True).tolist()
    with pytest.raises(smart_amd.SmartGpuError):
        smart_amd.iupac_sets(b"ACGT", ACGNT)


def _refused(rc):
    assert rc == ERR_ARG, rc
    assert engine.lib().smartgpu_last_error().decode() != ""


def test_iupac8_refusals():
    L = engine.lib()
    vals = np.zeros(8, dtype=np.uint8)
    vals[:5] = np.frombuffer(ACGNT, dtype=np.uint8)
    sets = np.full(8, 0xEE, dtype=np.uint8)
    P = np.frombuffer(b"GGAXCC", dtype=np.uint8).copy()
    _refused(L.smartgpu_iupac_sets8(vals.ctypes.data, 5, P.ctypes.data, 6, sets.ctypes.data))
    msg = L.smartgpu_last_error().decode()
    assert "position 3" in msg and "0x58" in msg, msg
    assert (sets == 0xEE).all()  # nothing written
    with pytest.raises(smart_amd.SmartGpuError, match="position 3"):
        smart_amd.iupac_sets(b"GGAXCC", ACGNT, wide=True)
    ok = np.frombuffer(b"GGATCC", dtype=np.uint8).copy()
    for k in (0, 9, -1):
        _refused(L.smartgpu_iupac_sets8(vals.ctypes.data, k, ok.ctypes.data, 6, sets.ctypes.data))
        assert str(k) in L.smartgpu_last_error().decode()
    _refused(L.smartgpu_iupac_sets8(None, 5, ok.ctypes.data, 6, sets.ctypes.data))
    _refused(L.smartgpu_iupac_sets8(vals.ctypes.data, 5, None, 6, sets.ctypes.data))
    _refused(L.smartgpu_iupac_sets8(vals.ctypes.data, 5, ok.ctypes.data, 6, None))
    assert (sets == 0xEE).all()
    with pytest.raises(smart_amd.SmartGpuError):
        smart_amd.iupac_sets(b"ACGT", bytes(range(9)), wide=True)


def test_refusals_that_need_no_device():
    """Without a device there is no handle: each call is decided before the first HIP call."""
    L = engine.lib()
    assert L.smartgpu_ptext_pack8(None) is None
    assert "NULL" in L.smartgpu_last_error().decode()
    vals = np.full(8, 0xEE, dtype=np.uint8)
    _refused(L.smartgpu_ptext_symbols8(None, vals.ctypes.data))
    assert (vals == 0xEE).all()
    _refused(L.smartgpu_iupac_sets8(vals.ctypes.data, 5, None, 3, vals.ctypes.data))  # NULL pattern


def test_integration_md_names_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + ["SMARTGPU_PTEXT_MAXVALUES", "ptext_layout8", "wide=True", "planes3_scan", "planes3_find", "planes3_pack"]:
        assert n in doc, n
