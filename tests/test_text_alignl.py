"""Starts and alignments of LONG edit-distance occurrences on byte texts (smartgpu_align_editl64,
smartgpu_align_editl_classes64: m <= 256, k <= 31) without a GPU: the declarations and bindings of both libraries, the source
registry, the documents, the refusals that are decided before the first HIP call, the ten-word vector oracle that
tests/test_text_alignl_gpu.py compares the library with, held to the by-definition oracle of tests/test_packed_align.py
(align_one), edit_cigar on ten-word rows, the band of alignl_band.hpp on the CPU under sanitizers
(tests/text_alignl_check.cpp), and the compiled kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

from test_packed_align import DEL, EQ, INS, SUB, align_one, replay
from test_packed_edit import byte_accepts

SYMBOLS = {"smartgpu_align_editl64": 11, "smartgpu_align_editl_classes64": 11}
PYTHON = ("align_editl", "align_editl_classes", "find_editl_align", "find_editl_classes_align")
ERR_ARG = -3
WORDS = 10  # SMARTGPU_ALIGNL_OPS_WORDS
NONE_START = np.uint64(2**64 - 1)
NONE_DIST = 255


# ---- the oracle ----------------------------------------------------------------------------------------------------------

def pack_opsl(ops):
    """The ten words of a list of operations: operation t in bits 2 * (t % 32) of word t // 32, the length in word 9."""
    assert len(ops) <= 32 * (WORDS - 1)
    w = [0] * WORDS
    for t, op in enumerate(ops):
        w[t // 32] |= op << (2 * (t % 32))
    w[WORDS - 1] = len(ops)
    return w


def unpack_opsl(row):
    w = [int(x) for x in row]
    assert len(w) == WORDS
    return [w[t // 32] >> (2 * (t % 32)) & 3 for t in range(w[WORDS - 1])]


def classes_accepts(classes):
    """accepts(i, symbols) of an (m, 32) array of byte classes: bit v % 8 of classes[i][v // 8] = position i accepts byte v"""
    classes = np.asarray(classes, dtype=np.uint8).reshape(-1, 32)
    return lambda i, sym: (classes[i][np.asarray(sym) >> 3] >> (np.asarray(sym) & 7) & 1).astype(bool)


def align_manyl(m, accepts, T, ends, k, off=0):
    """test_packed_align.align_many with ten words per entry and no bound on m and k but the words': align_one for many ends at
    once, every cell a numpy vector over the ends (column c holds the suffix of c symbols that ends at e: S[i][c] =
    ed(P[i..m), T[e-c+1 .. e])), the same choice of start and the same walk.  A row is filled without a loop over its
    columns: with A[c] = min(diagonal, the row below + 1) the recurrence S[i][c] = min(A[c], S[i][c-1] + 1) is
    S[i][c] = c + the running minimum of A[c'] - c' over c' <= c.  Returns what the call returns: (starts uint64, distances
    uint8, ops uint64 of shape (count, 10)), with the sentinel triple (2**64 - 1, 255, zeros) where D(e) > k.
    test_the_vector_oracle_is_the_definition holds it to align_one."""
    T = np.asarray(T)
    ends = np.asarray(ends, dtype=np.int64)
    E, W = len(ends), m + k
    ar = np.arange(E)
    length = np.minimum(W, ends - off + 1)                                   # columns that exist for each end
    sym = T[np.maximum(ends[None, :] - np.arange(W)[:, None], 0)]            # sym[c - 1]: the symbol column c adds
    acc = np.stack([accepts(i, sym) for i in range(m)]) if E else np.zeros((m, W, 0), dtype=bool)
    cols = np.arange(W + 1, dtype=np.int16)[:, None]
    S = np.zeros((m + 1, W + 1, E), dtype=np.int16)
    S[m] = cols
    A = np.empty((W + 1, E), dtype=np.int16)
    for i in range(m - 1, -1, -1):
        A[0] = m - i
        A[1:] = np.minimum(S[i + 1, :-1] + ~acc[i], S[i + 1, 1:] + 1)
        S[i] = np.minimum.accumulate(A - cols, axis=0) + cols
    row = np.where(np.arange(W + 1)[:, None] <= length[None, :], S[0], np.int16(30000))
    J = np.argmin(row, axis=0)                                               # the FIRST minimum: the shortest suffix, the largest start
    D = row[J, ar].astype(np.int64)
    hit = D <= k
    starts = np.where(hit, ends + 1 - J, 0).astype(np.uint64)
    starts[~hit] = NONE_START
    dist = np.where(hit, D, NONE_DIST).astype(np.uint8)
    words = np.zeros((E, WORDS), dtype=np.uint64)
    i, c, L = np.zeros(E, dtype=np.int64), np.where(hit, J, 0), np.zeros(E, dtype=np.uint64)
    i[~hit] = m                                                              # (non-occurrences: nothing to walk)
    for t in range(m + k):
        live = (i < m) | (c > 0)
        if not live.any():
            break
        i1, c1 = np.minimum(i + 1, m), np.maximum(c - 1, 0)
        here = S[np.minimum(i, m), c, ar]
        a = acc[np.minimum(i, m - 1), c1, ar]
        diag = live & (i < m) & (c > 0) & (S[i1, c1, ar] + ~a == here)
        dele = live & ~diag & (i < m) & (S[i1, c, ar] + 1 == here)
        ins = live & ~diag & ~dele
        op = np.where(diag, np.where(a, EQ, SUB), np.where(dele, DEL, INS)).astype(np.uint64)
        words[:, t // 32] |= np.where(live, op << np.uint64(2 * (t % 32)), np.uint64(0))
        L += live.astype(np.uint64)
        i = i + (diag | dele)
        c = c - (diag | ins)
    assert not ((i < m) | (c > 0)).any()                                     # every walk ended within m + k operations
    words[:, WORDS - 1] = np.where(hit, L, np.uint64(0))
    return starts, dist, words


def test_the_vector_oracle_is_the_definition():
    rng = np.random.default_rng(131)
    cases = 0
    for vals in ((65, 67, 71, 84), (0, 255), (7,)):
        for n, off in ((1, 0), (2, 0), (17, 0), (60, 0), (60, 13)):
            T = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]
            for m in (1, 2, 3, 8, 20, 33, 40):
                P = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), m)]
                if m <= n - off and rng.integers(0, 2):
                    P = T[n - m:].copy()
                    if m > 2:
                        P = np.delete(P, m // 2)  # a pattern that needs an insertion
                mm, accepts = len(P), byte_accepts(P)
                ends = np.arange(off, n)
                for k in (0, 2, 9, 31):
                    starts, dist, words = align_manyl(mm, accepts, T, ends, k, off)
                    for x, e in enumerate(ends.tolist()):
                        one = align_one(mm, accepts, T, e, k, off)
                        if one is None:
                            assert starts[x] == NONE_START and dist[x] == NONE_DIST and not words[x].any()
                            continue
                        s, d, ops = one
                        assert off <= s <= e + 1 and len(ops) <= mm + k and replay(ops, mm, accepts, T, s, e) == d
                        assert (int(starts[x]), int(dist[x]), words[x].tolist()) == (s, d, pack_opsl(ops)), (vals, n, off, mm, k, e)
                        assert unpack_opsl(words[x]) == ops
                    cases += 1
    assert cases == 3 * 5 * 7 * 4
    # a pattern of classes through classes_accepts: the singletons of P are P
    P = np.frombuffer(b"receive", dtype=np.uint8)
    T = np.frombuffer(b"Did you recieve the mesage?", dtype=np.uint8)
    got = align_manyl(7, classes_accepts(smart_amd.byte_classes(P)), T, [14], 2)
    assert (int(got[0][0]), int(got[1][0]), unpack_opsl(got[2][0])) == align_one(7, byte_accepts(P), T, 14, 2) == (8, 2, [EQ, EQ, EQ, SUB, SUB, EQ, EQ])


# ---- declarations, bindings, registry, documents -----------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()


def test_header_declares_the_calls():
    raw = open(os.path.join(ROOT, "include", "smartgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = set(re.findall(r"\b(smartgpu_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    assert re.search(r"^#define SMARTGPU_ALIGNL_OPS_WORDS 10$", text, flags=re.M)
    # the long find points at the new calls, and no longer says the short align call is all there is
    assert "ALIGNMENTS of long patterns on a byte text: smartgpu_align_editl64 below" in raw
    assert "on a byte text (smartgpu_align_edit64 stays at m <= 64, k <= 7)" not in raw
    assert "k_talignl.hip" in raw and "tools/talignl_probe.py" in raw and "text_editl_align" in raw


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
    with pytest.raises(ValueError):  # the classes forms go through _classes: the shape is checked before any call
        smart_amd.align_editl_classes(np.zeros((4, 31), dtype=np.uint8), None, 1, [3])
    with pytest.raises(ValueError):
        smart_amd.find_editl_classes_align(np.zeros(32, dtype=np.uint8), None, 1)


def test_sources_registry_has_the_unit_and_leaves_the_other_units_alone():
    assert [f for f in sources.UNITS["k_talignl"] if f.startswith("k_")] == ["k_talignl.hip"]
    for f in ("talignl.hpp", "alignl_band.hpp", "talign_host.hpp", "teditl_host.hpp", "edit_align.hpp"):
        assert f in sources.UNITS["k_talignl"], f
        assert os.path.exists(os.path.join(sources.CSRC, f)), f
    assert sources.KERNEL_UNIT["text_editl_align"] == "k_talignl"
    sha = sources.unit_sha256("k_talignl")
    assert sources.kernel_sha256("text_editl_align") == sha and sha not in (sources.unit_sha256("k_talign"), sources.unit_sha256("k_teditl"))
    assert sources.UNITS["k_talign"] == ("k_talign.hip", "talign.hpp", "talign_host.hpp", "tedit.hpp", "tedit_host.hpp", "edit_align.hpp", "edit_step.hpp",
                                         "planes.hpp")
    assert sources.UNITS["k_teditl"] == ("k_teditl.hip", "teditl.hpp", "teditl_host.hpp", "edit_block.hpp", "planes.hpp")
    assert sources.UNITS["k_peditl"] == ("k_peditl.hip", "peditl.hpp", "peditl_host.hpp", "edit_block.hpp", "planes.hpp")
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_talignl\b", makefile, flags=re.M)
    assert re.search(r"^UNITS\s*:=.*\balign_calls\b", makefile, flags=re.M)
    for h in ("talignl.hpp", "alignl_band.hpp", "call_host.hpp"):
        assert re.search(r"^HEADERS\s*:=.*\$\(HERE\)%s\b" % re.escape(h), makefile, flags=re.M), h
    # the exported functions live in the align calls' host unit, which shares its helpers with match_calls.cpp through a header
    unit = open(os.path.join(sources.CSRC, "align_calls.cpp")).read()
    defined = set(re.findall(r"^int smartgpu_([a-z0-9_]+)\(", unit, flags=re.M))
    assert defined == {"palign_edit64", "palign_sets_edit64", "align_edit64", "align_edit_classes64", "align_editl64", "align_editl_classes64"}
    shared = open(os.path.join(sources.CSRC, "call_host.hpp")).read()
    for helper in ("check_text_args", "check_align_lists", "ends_in_range", "text_table_stage", "teditl_stage"):
        assert re.search(r"\b%s\(" % helper, shared), helper
    for helper in ("upload_positions", "align_pieces"):  # the align unit's own
        assert not re.search(r"\b%s\(" % helper, shared), helper
    assert not os.path.exists(os.path.join(sources.CSRC, "alignl_calls.cpp")) and not os.path.exists(os.path.join(sources.CSRC, "align_host.hpp"))


def test_documents_name_every_symbol():
    names = list(SYMBOLS) + list(PYTHON) + ["SMARTGPU_ALIGNL_OPS_WORDS", "text_editl_align", "k_talignl.hip"]
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for n in names:
            assert n in text, (doc, n)
    results = open(os.path.join(ROOT, "profiles", "tedit", "RESULTS.md")).read()
    assert "Long patterns: starts and alignments" in results and "talignl_probe.py" in results
    assert os.path.exists(os.path.join(ROOT, "tools", "talignl_probe.py"))


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_classes"])
def test_refusals_that_need_no_device(kind):
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call, for
    the reason its line states, and writes nothing.  (An end outside a REAL range is refused in tests/test_text_alignl_gpu.py.)"""
    f = getattr(engine.lib(), "smartgpu_align_editl%s64" % kind)
    P = np.full(32 * 300, 1, dtype=np.uint8)
    ends = np.arange(8, dtype=np.uint64)
    starts = np.full(8, 77, dtype=np.uint64)
    dist = np.full(8, 7, dtype=np.uint8)
    ops = np.full(8 * WORDS, 5, dtype=np.uint64)
    call = lambda p, m, k, e, cnt, s: f(p, m, k, None, 0, 1000, e, cnt, s, dist.ctypes.data, ops.ctypes.data)  # noqa: E731
    _refused(call(None, 100, 9, ends.ctypes.data, 8, starts.ctypes.data), "classes is NULL" if kind else "P is NULL")
    _refused(call(P.ctypes.data, 0, 9, ends.ctypes.data, 8, starts.ctypes.data), "length 0 outside [1,256]")
    _refused(call(P.ctypes.data, 257, 9, ends.ctypes.data, 8, starts.ctypes.data), "length 257 outside [1,256]")
    _refused(call(P.ctypes.data, 100, 32, ends.ctypes.data, 8, starts.ctypes.data), "k = 32 edits, at most 31")
    _refused(call(P.ctypes.data, 100, 9, None, 8, starts.ctypes.data), "ends NULL with count > 0")
    _refused(call(P.ctypes.data, 100, 9, ends.ctypes.data, 8, None), "starts NULL with count > 0")
    _refused(call(P.ctypes.data, 100, 9, ends.ctypes.data, 8, starts.ctypes.data), "text handle is NULL")
    _refused(call(P.ctypes.data, 256, 31, ends.ctypes.data, 8, starts.ctypes.data), "text handle is NULL")  # the largest legal m and k pass the bounds
    _refused(call(P.ctypes.data, 100, 9, None, 0, None), "text handle is NULL")  # count == 0 excuses the NULL lists, not the NULL text
    assert ("align_editl%s64:" % kind) in engine.lib().smartgpu_last_error().decode()
    # the order of the short call: a missing list before the pattern's checks
    _refused(call(None, 0, 32, None, 8, starts.ctypes.data), "ends NULL with count > 0")
    assert (starts == 77).all() and (dist == 7).all() and (ops == 5).all() and (ends == np.arange(8)).all()


# ---- edit_cigar ----------------------------------------------------------------------------------------------------------

def test_edit_cigar_on_hand_written_ten_word_rows():
    row = lambda ops: np.array(pack_opsl(ops), dtype=np.uint64)  # noqa: E731
    assert smart_amd.edit_cigar(row([])) == ""
    assert smart_amd.edit_cigar(np.zeros(WORDS, dtype=np.uint64)) == ""  # an end that is no occurrence
    assert smart_amd.edit_cigar(row([EQ, EQ, EQ, SUB, SUB, EQ, EQ])) == "3=2X2="
    assert smart_amd.edit_cigar(row([DEL, EQ, SUB, EQ, EQ, EQ, EQ])) == "1D1=1X4="
    assert smart_amd.edit_cigar(row([DEL, EQ, INS]), sam=True) == "1I1=1D"
    # more than 96 operations, across the words' borders: runs that end at t = 31 / 32 and 63 / 64, the longest alignment
    long_ops = [EQ] * 31 + [SUB] + [INS] + [EQ] * 31 + [DEL] * 2 + [EQ] * 100 + [SUB] * 3 + [EQ] * 118
    assert len(long_ops) == 287
    assert smart_amd.edit_cigar(row(long_ops)) == "31=1X1I31=2D100=3X118="
    assert smart_amd.edit_cigar(row(long_ops), sam=True) == "31=1X1D31=2I100=3X118="
    assert unpack_opsl(row(long_ops)) == long_ops
    # three-word rows behave as before; other lengths are refused
    assert smart_amd.edit_cigar(np.array([0b0100, 0, 3 << 56], dtype=np.uint64)) == "1=1X1="
    for bad in (2, 4, 9, 11):
        with pytest.raises(ValueError):
            smart_amd.edit_cigar(np.zeros(bad, dtype=np.uint64))
    with pytest.raises(ValueError):  # a length the nine words cannot hold
        smart_amd.edit_cigar(np.array([0] * 9 + [289], dtype=np.uint64))


# ---- the band on the CPU ---------------------------------------------------------------------------------------------------

def test_cell_rule_band_decisions_and_traceback_on_the_host(tmp_path):
    """tests/text_alignl_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process: alignl_band.hpp stepped
    lane by lane as the kernel steps it — the word-major table of the reversed pattern, bytes from the 73-dword window, the
    packed decisions, the key reduction, the walk — against a scalar full-matrix DP written out in the program: start,
    distance, every operation and the packing."""
    exe = tmp_path / "text_alignl_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "text_alignl_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # the cell rule + per length: 4 alphabets x 5 values of k, + (both kinds of end, every phase, clipped ends seen); 11 lengths
    assert r.returncode == 0 and failures == 0 and cases == 1 + 11 * (4 * 5 + 1), r.stdout[-4000:] + r.stderr[-2000:]


def test_the_unit_holds_six_kernels_without_scratch_and_static_lds():
    """text_editl_align for 2, 4 and 8 mask dwords, with and without the decisions: exactly six kernels of the k_talignl code
    object, each with ScratchSize 0 (-Rpass-analysis=kernel-resource-usage).  The LDS is static, so the compiler reports all
    of it: table + four windows of 73 dwords + (with ops) four waves x 17 x 64 dwords of decisions."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_talignl.hip")]
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
    assert len([k for k in usage if "text_editl_align" in k]) == 6, sorted(usage)
    text = open(os.path.join(sources.CSRC, "k_talignl.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(\(text_editl_align<w_, o_>\), dim3\(grid\), dim3\(kTAlignlT\), 0, stream, a\);", text)  # no dynamic LDS
    assert text.count("__syncthreads()") == 2 and text.index("__syncthreads();") < text.index("for (uint64_t idx")  # one barrier (and its mention), before the loop
    for words in (2, 4, 8):
        for ops in (0, 1):
            mine = [k for k in usage if re.search(r"text_editl_alignILi%dELb%dEE" % (words, ops), k)]
            assert len(mine) == 1, (words, ops, sorted(usage))
            lds = 4 * (256 * words + 4 * 73 + (4 * 17 * 64 if ops else 0))
            assert lds <= 65536
            assert usage[mine[0]] == {"scratch": 0, "lds": lds}, (mine[0], usage[mine[0]], lds)
