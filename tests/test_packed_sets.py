"""Set patterns on packed texts (smartgpu_psearch_sets64, smartgpu_pfind_sets64, smartgpu_iupac_sets) without a GPU: the
declarations, the bindings of both libraries, the source registry, the documentation, the refusals that are decided before
the first HIP call, the IUPAC table, and the compiled kernels planes_sets_scan / planes_sets_find."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_psearch_sets64": 8, "smartgpu_pfind_sets64": 8, "smartgpu_iupac_sets": 5}
ERR_ARG = -3

# the bases every IUPAC nucleotide letter accepts
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def test_header_declares_the_three_calls():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
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
            assert f.argtypes is not None and f.restype is ctypes.c_int, (path, n)  # the engine gave it a prototype
            assert len(f.argtypes) == nargs, (path, n)


def test_python_functions_exist():
    for name in ("psearch_sets", "pfind_sets", "iupac_sets"):
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)
    assert callable(smart_amd.PackedText.iupac)


def test_sources_registry_names_both_kernels():
    for k in ("planes_sets_scan", "planes_sets_find"):
        assert sources.KERNEL_UNIT[k] == "k_planes"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_planes") == sources.kernel_sha256("planes_scan")


def test_integration_md_names_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + ["psearch_sets", "pfind_sets", "iupac_sets", "PackedText.iupac"]:
        assert n in doc, n


def _refused(rc):
    assert rc == ERR_ARG, rc
    assert engine.lib().smartgpu_last_error().decode() != ""


def test_refusals_that_need_no_device():
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call."""
    L = engine.lib()
    S = np.full(4201, 1, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    c = ctypes.c_uint64(77)
    pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    times = (ctypes.byref(pre), ctypes.byref(run))
    _refused(L.smartgpu_psearch_sets64(None, 4, None, 0, 100, ctypes.byref(c), *times))                   # sets == NULL
    _refused(L.smartgpu_psearch_sets64(S.ctypes.data, 0, None, 0, 100, ctypes.byref(c), *times))          # m = 0
    _refused(L.smartgpu_psearch_sets64(S.ctypes.data, 4201, None, 0, 5000, ctypes.byref(c), *times))      # m > SMARTGPU_XSIZE
    _refused(L.smartgpu_psearch_sets64(S.ctypes.data, 4, None, 0, 100, ctypes.byref(c), *times))          # NULL text (and with it: any range)
    _refused(L.smartgpu_psearch_sets64(S.ctypes.data, 4, None, 1 << 40, 100, ctypes.byref(c), *times))    # a range outside the text
    _refused(L.smartgpu_psearch_sets64(S.ctypes.data, 4, None, 0, 100, None, *times))                     # count == NULL
    assert c.value == 77 and pre.value == -1.0 and run.value == -2.0  # a refused call writes nothing
    _refused(L.smartgpu_pfind_sets64(None, 4, None, 0, 100, out.ctypes.data, 8, ctypes.byref(c)))         # sets == NULL
    _refused(L.smartgpu_pfind_sets64(S.ctypes.data, 0, None, 0, 100, out.ctypes.data, 8, ctypes.byref(c)))
    _refused(L.smartgpu_pfind_sets64(S.ctypes.data, 4201, None, 0, 5000, out.ctypes.data, 8, ctypes.byref(c)))
    _refused(L.smartgpu_pfind_sets64(S.ctypes.data, 4, None, 0, 100, out.ctypes.data, 8, ctypes.byref(c)))  # NULL text
    _refused(L.smartgpu_pfind_sets64(S.ctypes.data, 4, None, 1 << 40, 100, out.ctypes.data, 8, ctypes.byref(c)))
    _refused(L.smartgpu_pfind_sets64(S.ctypes.data, 4, None, 0, 100, out.ctypes.data, 8, None))           # count == NULL
    _refused(L.smartgpu_pfind_sets64(S.ctypes.data, 4, None, 0, 100, None, 8, ctypes.byref(c)))           # positions == NULL, cap > 0
    assert c.value == 77 and not out.any()


def expected_sets(pattern, values):
    """The table written out: bit c of sets[j] = the base values[c] stands for is accepted by letter j."""
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


def test_iupac_all_letters_both_cases():
    letters = "".join(IUPAC)
    for pattern in (letters, letters.lower()):
        got = smart_amd.iupac_sets(pattern.encode(), b"ACGT")
        assert got.dtype == np.uint8
        # A=1 C=2 G=4 T=8 U=8 R=5 Y=10 S=6 W=9 K=12 M=3 B=14 D=13 H=11 V=7 N=15
        assert got.tolist() == [1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15]
        assert got.tolist() == expected_sets(pattern, b"ACGT")
    assert smart_amd.iupac_sets("GGNCC", b"ACGT").tolist() == [4, 4, 15, 2, 2]  # a str is taken as its bytes


def test_iupac_other_value_sets():
    letters = "".join(IUPAC)
    low = smart_amd.iupac_sets(letters.encode(), b"acgt")  # lower-case text values
    assert low.tolist() == smart_amd.iupac_sets(letters.encode(), b"ACGT").tolist()
    three = smart_amd.iupac_sets(b"GSACTN", b"ACT")  # a three-value text: no G
    assert three.tolist() == [0, 2, 1, 2, 4, 7]
    assert smart_amd.iupac_sets(letters.encode(), b"ACT").tolist() == expected_sets(letters, b"ACT")
    assert smart_amd.iupac_sets(b"UuTt", b"ACGT").tolist() == [8, 8, 8, 8]                  # U is T in the pattern
    assert smart_amd.iupac_sets(b"TUWN", b"ACGU").tolist() == [8, 8, 9, 15]                 # and among the text's values
    assert smart_amd.iupac_sets(b"TA", b"AT").tolist() == [2, 1]                            # codes follow the values' order
    assert not smart_amd.iupac_sets(letters.encode(), (0, 1, 2, 3)).any()                   # values that are no bases
    assert smart_amd.iupac_sets(b"", b"ACGT").tolist() == []


def test_iupac_refusals():
    L = engine.lib()
    vals = np.frombuffer(b"ACGT", dtype=np.uint8).copy()
    sets = np.full(8, 0xEE, dtype=np.uint8)
    P = np.frombuffer(b"GGAXCC", dtype=np.uint8).copy()
    _refused(L.smartgpu_iupac_sets(vals.ctypes.data, 4, P.ctypes.data, 6, sets.ctypes.data))
    msg = L.smartgpu_last_error().decode()
    assert "position 3" in msg and "0x58" in msg, msg
    assert (sets == 0xEE).all()  # nothing written
    with pytest.raises(smart_amd.SmartGpuError, match="position 3"):
        smart_amd.iupac_sets(b"GGAXCC", b"ACGT")
    with pytest.raises(smart_amd.SmartGpuError, match="position 0"):
        smart_amd.iupac_sets(bytes([0]), b"ACGT")
    ok = np.frombuffer(b"GGATCC", dtype=np.uint8).copy()
    for k in (0, 5, -1):
        _refused(L.smartgpu_iupac_sets(vals.ctypes.data, k, ok.ctypes.data, 6, sets.ctypes.data))
        assert str(k) in L.smartgpu_last_error().decode()
    _refused(L.smartgpu_iupac_sets(None, 4, ok.ctypes.data, 6, sets.ctypes.data))
    _refused(L.smartgpu_iupac_sets(vals.ctypes.data, 4, None, 6, sets.ctypes.data))
    _refused(L.smartgpu_iupac_sets(vals.ctypes.data, 4, ok.ctypes.data, 6, None))
    assert (sets == 0xEE).all()
    with pytest.raises(smart_amd.SmartGpuError):
        smart_amd.iupac_sets(b"ACGT", b"")
    with pytest.raises(smart_amd.SmartGpuError):
        smart_amd.iupac_sets(b"ACGT", b"ACGTU")


def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """planes_sets_scan and planes_sets_find, for one and two planes, are kernels of the k_planes code object, each with
    ScratchSize 0 and no static LDS (-Rpass-analysis=kernel-resource-usage, as tests/test_build.py reads it)."""
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
            mine = [k for k in usage if re.search(r"planes_sets_%sILi%dEE" % (kind, planes), k)]
            assert len(mine) == 1, (kind, planes, sorted(usage))
            assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
