"""Edit distance on packed texts (smartgpu_psearch_edit64, smartgpu_pfind_edit64 and their sets forms) without a GPU: the
ORACLE the GPU tests compare with (Sellers' DP, row by row in numpy) against a plain triple-loop DP, the declarations and
bindings of both libraries, the source registry, the documentation, the refusals that are decided before the first HIP call,
the recurrence step and the masks on the CPU under sanitizers (tests/packed_edit_check.cpp), and the compiled kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

SYMBOLS = {"smartgpu_psearch_edit64": 9, "smartgpu_pfind_edit64": 10, "smartgpu_psearch_sets_edit64": 9, "smartgpu_pfind_sets_edit64": 10}
ERR_ARG = -3
# what k_pedit.hip chose (pedit.hpp kEditRun; test_the_restated_run_length_is_the_kernels): end positions a lane owns, and
# with them those of a wave (64 lanes) and of a workgroup (256 lanes)
RUN = 128
WAVE_RUN = 64 * RUN
WG_RUN = 256 * RUN


# ---- the oracle ------------------------------------------------------------------------------------------------------

def byte_accepts(P):
    """accepts(i, R): which symbols of the range R pattern position i matches — a byte pattern."""
    return lambda i, R: R == P[i]


def set_accepts(sets, values):
    """The same for a SET pattern over a text whose values (ascending) are `values`: bit c of sets[i] accepts values[c]."""
    code = np.full(256, 255, dtype=np.uint8)
    code[np.asarray(values, dtype=np.uint8)] = np.arange(len(values), dtype=np.uint8)

    def accepts(i, R):
        c = code[R]
        return (c < len(values)) & ((int(sets[i]) >> np.minimum(c, 7)) & 1).astype(bool)
    return accepts


def edit_row(m, accepts, T, off=0, n=None):
    """D(e) for off <= e < off + n as int32: the last row of Sellers' DP on the range ALONE — D[0][*] = 0, the column before
    the range D[i] = i.  Row by row: the diagonal and vertical terms as one vector minimum, the horizontal term as a prefix
    minimum (D[c] = min over c' <= c of A[c'] + c - c').  m vector passes, no loop over the text."""
    n = len(T) - off if n is None else n
    R = np.asarray(T[off:off + n])
    idx = np.arange(n + 1, dtype=np.int32)
    D = np.zeros(n + 1, dtype=np.int32)  # index c + 1 holds column c of the range; index 0 the column before it
    for i in range(m):
        A = np.empty(n + 1, dtype=np.int32)
        A[0] = i + 1
        np.minimum(D[:-1] + (~accepts(i, R)), D[1:] + 1, out=A[1:])
        D = np.minimum.accumulate(A - idx) + idx
    return D[1:]


def edit_occurrences(m, accepts, T, k, off=0, n=None):
    """(ascending end positions relative to symbol 0 as uint64, their distances as uint8): every e with D(e) <= k."""
    D = edit_row(m, accepts, T, off, n)
    at = np.flatnonzero(D <= k)
    return (at + off).astype(np.uint64), D[at].astype(np.uint8)


def plain_dp(P_accepts_symbol, m, T):
    """The definition, cell by cell: D[i][c] = min(D[i-1][c-1] + mismatch, D[i-1][c] + 1, D[i][c-1] + 1)."""
    n = len(T)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        D[i][0] = i
    for i in range(1, m + 1):
        for c in range(1, n + 1):
            D[i][c] = min(D[i - 1][c - 1] + (0 if P_accepts_symbol(i - 1, int(T[c - 1])) else 1), D[i - 1][c] + 1, D[i][c - 1] + 1)
    return D[m][1:]


def test_the_oracle_equals_the_plain_dp():
    rng = np.random.default_rng(41)
    cases = 0
    for vals in ((65, 67, 71, 84), (0, 255), (7,)):
        for n in (1, 2, 5, 17, 40):
            T = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]
            for m in (1, 2, 3, 8, 20, 45):
                P = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), m)]
                if m <= n and rng.integers(0, 2):
                    P = T[n - m:].copy()
                if rng.integers(0, 3) == 0:
                    P[rng.integers(0, m)] = ord("N")  # a byte the text does not hold
                assert edit_row(m, byte_accepts(P), T).tolist() == plain_dp(lambda i, s: P[i] == s, m, T), (vals, n, m)
                sets = rng.integers(0, 1 << len(vals), m).astype(np.uint8)
                want = plain_dp(lambda i, s: bool(sets[i] >> vals.index(s) & 1), m, T)
                assert edit_row(m, set_accepts(sets, vals), T).tolist() == want, (vals, n, m, "sets")
                cases += 2
    # a sub-range is the DP on the substring
    T = np.asarray((65, 67, 71, 84), dtype=np.uint8)[rng.integers(0, 4, 40)]
    P = T[10:18].copy()
    assert edit_row(8, byte_accepts(P), T, 12, 20).tolist() == plain_dp(lambda i, s: P[i] == s, 8, T[12:32])
    assert edit_row(8, byte_accepts(P), T, 12, 20)[5] > 0 and edit_row(8, byte_accepts(P), T)[17] == 0
    pos, dist = edit_occurrences(8, byte_accepts(P), T, 0)
    assert 17 in pos.tolist() and not dist.any() and pos.dtype == np.uint64 and dist.dtype == np.uint8
    assert cases == 3 * 5 * 6 * 2


# ---- declarations, bindings, registry, documents -----------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def test_header_declares_the_calls_and_the_bound():
    text = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    assert re.search(r"^#define\s+SMARTGPU_PEDIT_MAXM\s+64\b", text, flags=re.M)


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
    for name in ("psearch_edit", "pfind_edit", "psearch_sets_edit", "pfind_sets_edit"):
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_has_the_unit_and_leaves_the_planes_unit_alone():
    assert [f for f in sources.UNITS["k_pedit"] if f.startswith("k_")] == ["k_pedit.hip"]
    for f in ("pedit.hpp", "edit_step.hpp"):
        assert f in sources.UNITS["k_pedit"], f
    for k in ("planes_edit_scan", "planes_edit_find"):
        assert sources.KERNEL_UNIT[k] == "k_pedit"
        assert sources.kernel_sha256(k) == sources.unit_sha256("k_pedit") != sources.unit_sha256("k_planes")
    assert sources.UNITS["k_planes"] == ("k_planes.hip", "planes.hpp")
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_pedit\b", makefile, flags=re.M)


def test_the_restated_run_length_is_the_kernels():
    text = open(os.path.join(sources.CSRC, "pedit.hpp")).read()
    assert re.search(r"constexpr uint32_t kEditRun = %d;" % RUN, text)


def test_documents_name_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + ["psearch_edit", "pfind_edit", "psearch_sets_edit", "pfind_sets_edit", "SMARTGPU_PEDIT_MAXM"]:
        assert n in doc, n
    assert "smartgpu_psearch_edit64" in open(os.path.join(ROOT, "README.md")).read()
    assert "planes_edit_scan" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    """-3 and a message that names the reason (`says`), so that each case is refused for what its comment states."""
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_sets"])
def test_refusals_that_need_no_device(kind):
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call.
    (A range outside a REAL text and a set that names a code the text does not hold are refused in
    tests/test_packed_edit_gpu.py; here the NULL handle is what those cases meet.)"""
    L = engine.lib()
    what = "sets is NULL" if kind else "P is NULL"
    P = np.full(100, 1, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    dist = np.zeros(8, dtype=np.uint8)
    c = ctypes.c_uint64(77)
    pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    times = (ctypes.byref(pre), ctypes.byref(run))
    count = getattr(L, "smartgpu_psearch%s_edit64" % kind)
    _refused(count(None, 4, 1, None, 0, 100, ctypes.byref(c), *times), what)
    _refused(count(P.ctypes.data, 0, 1, None, 0, 100, ctypes.byref(c), *times), "length 0 outside [1,64]")
    _refused(count(P.ctypes.data, 65, 1, None, 0, 100, ctypes.byref(c), *times), "length 65 outside [1,64]")  # m > SMARTGPU_PEDIT_MAXM
    _refused(count(P.ctypes.data, 4, 8, None, 0, 100, ctypes.byref(c), *times), "k = 8 ")                     # k > SMARTGPU_PMIS_MAX
    _refused(count(P.ctypes.data, 4, 1, None, 0, 100, ctypes.byref(c), *times), "handle is NULL")
    _refused(count(P.ctypes.data, 64, 7, None, 1 << 40, 100, ctypes.byref(c), *times), "handle is NULL")      # a range outside the text
    _refused(count(P.ctypes.data, 4, 1, None, 0, 100, None, *times), "handle is NULL")                        # and count == NULL
    assert c.value == 77 and pre.value == -1.0 and run.value == -2.0  # a refused call writes nothing
    f = getattr(L, "smartgpu_pfind%s_edit64" % kind)
    find = lambda p, m, k, off, n, pos, cap, cnt: f(p, m, k, None, off, n, pos, dist.ctypes.data, cap, cnt)  # noqa: E731
    _refused(find(None, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), what)
    _refused(find(P.ctypes.data, 0, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "length 0 outside [1,64]")
    _refused(find(P.ctypes.data, 65, 1, 0, 5000, out.ctypes.data, 8, ctypes.byref(c)), "length 65 outside [1,64]")
    _refused(find(P.ctypes.data, 4, 8, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "k = 8 ")
    _refused(find(P.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 1 << 40, 100, out.ctypes.data, 8, ctypes.byref(c)), "handle is NULL")
    _refused(find(P.ctypes.data, 4, 1, 0, 100, out.ctypes.data, 8, None), "handle is NULL")                   # and count == NULL
    _refused(find(P.ctypes.data, 4, 1, 0, 100, None, 8, ctypes.byref(c)), "ends NULL")                        # ends == NULL, cap > 0
    assert c.value == 77 and not out.any() and not dist.any()


# ---- the recurrence and the masks on the CPU ---------------------------------------------------------------------------

def test_recurrence_step_and_masks_on_the_host(tmp_path):
    """tests/packed_edit_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process: edit_step for WORDS = 1
    and 2 over random texts on 1 to 4 values against a scalar DP, every column's score — m = 1, 2, 31, 32 (and 33, 63, 64 on
    two dwords), byte patterns and set patterns, the all-equal pattern on an all-equal text (the carry runs through every bit),
    fresh starts at e - (m + k) for k = 0, 1, 3, 7 against the full DP wherever the full value is <= k (and > k elsewhere) —
    and edit_peq_pattern / edit_peq_sets bit by bit: foreign bytes and empty sets get no bit, a full set a bit in every held
    code's mask, a set bit at or above nvalues is refused and its position returned."""
    exe = tmp_path / "packed_edit_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "packed_edit_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # per length: 4 alphabets x 2 kinds of pattern x (the scores + 4 fresh starts) + the all-equal case; 4 lengths on one
    # dword, 7 on two; the masks: 4 alphabets x 5 lengths x 4 checks
    assert r.returncode == 0 and failures == 0 and cases == (4 + 7) * (4 * 2 * 5 + 1) + 4 * 5 * 4, r.stdout[-4000:] + r.stderr[-2000:]


def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """planes_edit_scan and planes_edit_find, for one and two planes and one and two dwords, are kernels of the k_pedit code
    object, each with ScratchSize 0 and no static LDS (-Rpass-analysis=kernel-resource-usage, as tests/test_packed_mis.py
    reads it)."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_pedit.hip")]
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
            for words in (1, 2):
                mine = [k for k in usage if re.search(r"planes_edit_%sILi%dELi%dEE" % (kind, planes, words), k)]
                assert len(mine) == 1, (kind, planes, words, sorted(usage))
                assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
