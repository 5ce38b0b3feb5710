"""Set patterns with mismatches on packed texts (smartgpu_psearch_sets_mis64, smartgpu_pfind_sets_mis64) and the reverse
complement of an IUPAC pattern (smartgpu_iupac_revcomp) without a GPU: the declarations, the bindings of both libraries, the
source registry, the documentation, the refusals that are decided before the first HIP call, the letter map, and the
compiled kernels planes_sets_mis_scan / planes_sets_mis_find."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_psearch_sets_mis64": 9, "smartgpu_pfind_sets_mis64": 10, "smartgpu_iupac_revcomp": 3}
ERR_ARG = -3
LETTERS = "ACGTURYSWKMBDHVN"
ACGT = (65, 67, 71, 84)


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def test_header_declares_the_calls_and_offers_the_feature():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    assert not re.search(r"NOT offered:\s*set patterns with mismatches", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", code))
    for n in SYMBOLS:
        assert n in names, n
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert not re.search(r"NOT offered:\s*set patterns with mismatches", readme)


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
    for name in ("psearch_sets_mis", "pfind_sets_mis", "iupac_revcomp"):
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_names_both_kernels():
    for k in ("planes_sets_mis_scan", "planes_sets_mis_find"):
        assert sources.KERNEL_UNIT[k] == "k_planes"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_planes") == sources.kernel_sha256("planes_scan")


def test_integration_md_names_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + ["psearch_sets_mis", "pfind_sets_mis", "iupac_revcomp"]:
        assert n in doc, n


def _refused(rc, says):
    """-3 and a message that names the reason (`says`), so that each case is refused for what its comment states."""
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


def test_refusals_that_need_no_device():
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call.
    (A range outside a REAL text and a set beyond the text's values are refused in tests/test_packed_sets_mis_gpu.py.)"""
    L = engine.lib()
    S = np.full(4201, 1, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    mis = np.zeros(8, dtype=np.uint8)
    c = ctypes.c_uint64(77)
    pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    times = (ctypes.byref(pre), ctypes.byref(run))
    _refused(L.smartgpu_psearch_sets_mis64(None, 4, 1, None, 0, 100, ctypes.byref(c), *times), "sets is NULL")
    _refused(L.smartgpu_psearch_sets_mis64(S.ctypes.data, 0, 1, None, 0, 100, ctypes.byref(c), *times), "length 0 ")
    _refused(L.smartgpu_psearch_sets_mis64(S.ctypes.data, 4201, 1, None, 0, 5000, ctypes.byref(c), *times), "length 4201 ")  # m > SMARTGPU_XSIZE
    _refused(L.smartgpu_psearch_sets_mis64(S.ctypes.data, 4, 8, None, 0, 100, ctypes.byref(c), *times), "k = 8 ")         # k > SMARTGPU_PMIS_MAX
    _refused(L.smartgpu_psearch_sets_mis64(S.ctypes.data, 4, 1, None, 0, 100, ctypes.byref(c), *times), "handle is NULL")
    _refused(L.smartgpu_psearch_sets_mis64(S.ctypes.data, 4, 1, None, 0, 100, None, *times), "handle is NULL")             # and count == NULL
    assert c.value == 77 and pre.value == -1.0 and run.value == -2.0  # a refused call writes nothing
    find = lambda s, m, k, off, n, pos, cap, cnt: L.smartgpu_pfind_sets_mis64(s, m, k, None, off, n, pos, mis.ctypes.data, cap, cnt)  # noqa: E731
    _refused(find(None, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "sets is NULL")
    _refused(find(S.ctypes.data, 0, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "length 0 ")
    _refused(find(S.ctypes.data, 4201, 1, 0, 5000, out.ctypes.data, 8, ctypes.byref(c)), "length 4201 ")
    _refused(find(S.ctypes.data, 4, 8, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "k = 8 ")
    _refused(find(S.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(S.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, None), "handle is NULL")                                 # and count == NULL
    _refused(find(S.ctypes.data, 4, 1, 0, 100, None, 8, ctypes.byref(c)), "positions NULL")                                 # positions == NULL, cap > 0
    assert c.value == 77 and not out.any() and not mis.any()


def test_revcomp_of_a_primer_and_the_involution():
    assert smart_amd.iupac_revcomp("GGNCCWR") == "YWGGNCC"
    assert smart_amd.iupac_revcomp(b"GGNCCWR") == b"YWGGNCC"
    assert smart_amd.iupac_revcomp("") == ""
    no_u = LETTERS.replace("U", "")
    for letters in (no_u, no_u.lower(), "aCgTrYkMbVdHsWn"):
        once = smart_amd.iupac_revcomp(letters)
        assert len(once) == len(letters) and once != letters
        assert smart_amd.iupac_revcomp(once) == letters, letters
        assert [ch.isupper() for ch in once] == [ch.isupper() for ch in letters[::-1]]  # case is preserved
    want = {"A": "T", "T": "A", "C": "G", "G": "C", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D",
            "S": "S", "W": "W", "N": "N", "U": "A"}
    for x in LETTERS:
        assert smart_amd.iupac_revcomp(x) == want[x], x
        assert smart_amd.iupac_revcomp(x.lower()) == want[x].lower(), x
    # U reads as T: its complement is A, and back comes T
    assert smart_amd.iupac_revcomp("ACGU") == "ACGT" and smart_amd.iupac_revcomp("u") == "a"
    assert smart_amd.iupac_revcomp(smart_amd.iupac_revcomp("GAUUACA")) == "GATTACA"


def test_revcomp_refuses_a_bad_byte_and_writes_nothing():
    L = engine.lib()
    P = np.frombuffer(b"ACGXT", dtype=np.uint8).copy()
    out = np.full(5, 7, dtype=np.uint8)
    _refused(L.smartgpu_iupac_revcomp(P.ctypes.data, 5, out.ctypes.data), "position 3")
    assert "0x58" in L.smartgpu_last_error().decode()
    assert (out == 7).all()
    with pytest.raises(smart_amd.SmartGpuError):
        smart_amd.iupac_revcomp("AC-GT")
    _refused(L.smartgpu_iupac_revcomp(None, 5, out.ctypes.data), "NULL")
    _refused(L.smartgpu_iupac_revcomp(P.ctypes.data, 5, None), "NULL")
    # in place
    Q = np.frombuffer(b"GGNCCWR", dtype=np.uint8).copy()
    assert L.smartgpu_iupac_revcomp(Q.ctypes.data, 7, Q.ctypes.data) == 0 and Q.tobytes() == b"YWGGNCC"


def test_revcomp_is_the_complement_permuted_set():
    """Over the values ACGT the complement swaps codes 0 <-> 3 and 1 <-> 2: the set of a letter's reverse complement is the
    letter's set with its four bits reversed."""
    for x in LETTERS + LETTERS.lower():
        s = int(smart_amd.iupac_sets(x, ACGT)[0])
        permuted = sum(1 << (3 - c) for c in range(4) if s >> c & 1)
        assert int(smart_amd.iupac_sets(smart_amd.iupac_revcomp(x), ACGT)[0]) == permuted, x
    # and a whole pattern: reversed as well
    P = "GGNCCWRTATAWAW"
    s = smart_amd.iupac_sets(P, ACGT)
    want = [sum(1 << (3 - c) for c in range(4) if int(v) >> c & 1) for v in s[::-1]]
    assert smart_amd.iupac_sets(smart_amd.iupac_revcomp(P), ACGT).tolist() == want


def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """planes_sets_mis_scan and planes_sets_mis_find, for one and two planes and counters of 1, 2 and 3 bits — 12 kernels of
    the k_planes code object — each with ScratchSize 0 and no static LDS (-Rpass-analysis=kernel-resource-usage, as
    tests/test_packed_mis.py reads it)."""
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
    seen = 0
    for kind in ("scan", "find"):
        for planes in (1, 2):
            for bits in (1, 2, 3):
                mine = [k for k in usage if re.search(r"planes_sets_mis_%sILi%dELi%dEE" % (kind, planes, bits), k)]
                assert len(mine) == 1, (kind, planes, bits, sorted(usage))
                assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
                seen += 1
    assert seen == 12
