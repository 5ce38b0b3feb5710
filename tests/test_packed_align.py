"""Starts and alignments of edit-distance occurrences on packed texts (smartgpu_palign_edit64, smartgpu_palign_sets_edit64)
without a GPU: the ORACLE the GPU tests compare with — a plain DP of the suffix distances, independent of the bit-vector
code — against the distances of edit_row, the declarations and bindings of both libraries, the source registry, the
documentation, the refusals that are decided before the first HIP call, edit_cigar, the shared header on the CPU under
sanitizers (tests/packed_align_check.cpp), and the compiled kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import smart_amd
from smart_amd import engine, sources

from test_packed_edit import byte_accepts, edit_row, set_accepts

SYMBOLS = {"smartgpu_palign_edit64": 11, "smartgpu_palign_sets_edit64": 11}
ERR_ARG = -3
NONE_START = np.uint64(2**64 - 1)
NONE_DIST = 255
EQ, SUB, INS, DEL = 0, 1, 2, 3


# ---- the oracle ------------------------------------------------------------------------------------------------------

def align_one(m, accepts, T, e, k, off=0):
    """THIS IS THE DEFINITION (include/smartgpu.h, smartgpu_palign_edit64), cell by cell in Python lists.  For the end e of
    the range that starts at off it fills the scalar matrix of the pattern against W = T[max(off, e-m-k+1) .. e],
        S[i][p] = ed(P[i..m), W[p..]),
    and derives from it D(e) = min over p of S[0][p], the LARGEST minimising start, and — when D(e) <= k — the operations:
    from (i, p) = (0, start) take the first that applies of the diagonal ('=' 0 / 'X' 1) when S[i+1][p+1] + cost == S[i][p],
    'D' 3 when S[i+1][p] + 1 == S[i][p], else 'I' 2.  Returns (start relative to symbol 0, D, list of operations), or None
    when the minimum over the window exceeds k (then D(e) > k: a match within k has at most m + k symbols)."""
    lo = max(off, e - m - k + 1)
    Wt = np.asarray(T[lo:e + 1])
    W = len(Wt)
    acc = [accepts(i, Wt).tolist() for i in range(m)]
    S = [[0] * (W + 1) for _ in range(m + 1)]
    for p in range(W + 1):
        S[m][p] = W - p
    for i in range(m - 1, -1, -1):
        S[i][W] = m - i
        for p in range(W - 1, -1, -1):
            S[i][p] = min(S[i + 1][p + 1] + (0 if acc[i][p] else 1), S[i + 1][p] + 1, S[i][p + 1] + 1)
    D = min(S[0])
    if D > k:
        return None
    start = max(p for p in range(W + 1) if S[0][p] == D)
    ops, i, p = [], 0, start
    while i < m or p < W:
        if i < m and p < W and S[i + 1][p + 1] + (0 if acc[i][p] else 1) == S[i][p]:
            ops.append(EQ if acc[i][p] else SUB)
            i, p = i + 1, p + 1
        elif i < m and S[i + 1][p] + 1 == S[i][p]:
            ops.append(DEL)
            i += 1
        else:
            ops.append(INS)
            p += 1
    return lo + start, D, ops


def pack_ops(ops):
    """The three words of a list of operations: operation t in bits 2 * (t % 32) of word t // 32, the length in the top byte."""
    w = [0, 0, 0]
    for t, op in enumerate(ops):
        w[t // 32] |= op << (2 * (t % 32))
    w[2] |= len(ops) << 56
    return w


def unpack_ops(row):
    w = [int(x) for x in row]
    return [w[t // 32] >> (2 * (t % 32)) & 3 for t in range(w[2] >> 56)]


def align_many(m, accepts, T, ends, k, off=0):
    """align_one for many ends at once: the same matrix, cell by cell, every cell a numpy vector over the ends (column c
    holds the suffix of c symbols that ends at e: S[i][c] = ed(P[i..m), T[e-c+1 .. e])), the same choice of start and
    the same walk.  Returns what the call returns: (starts uint64, distances uint8, ops uint64 of shape (count, 3)), with the
    sentinel triple (2**64 - 1, 255, zeros) where D(e) > k.  test_the_oracle_against_edit_row_and_the_vector_oracle_is_the_definition holds it to
    align_one."""
    T = np.asarray(T)
    ends = np.asarray(ends, dtype=np.int64)
    E, W = len(ends), m + k
    ar = np.arange(E)
    length = np.minimum(W, ends - off + 1)                                   # columns that exist for each end
    sym = T[np.maximum(ends[None, :] - np.arange(W)[:, None], 0)]            # sym[c - 1]: the symbol column c adds
    acc = np.stack([accepts(i, sym) for i in range(m)]) if E else np.zeros((m, W, 0), dtype=bool)
    S = np.zeros((m + 1, W + 1, E), dtype=np.int16)
    S[m] = np.arange(W + 1, dtype=np.int16)[:, None]
    for i in range(m - 1, -1, -1):
        S[i, 0] = m - i
        for c in range(1, W + 1):
            S[i, c] = np.minimum(np.minimum(S[i + 1, c - 1] + ~acc[i, c - 1], S[i + 1, c] + 1), S[i, c - 1] + 1)
    row = np.where(np.arange(W + 1)[:, None] <= length[None, :], S[0], np.int16(30000))
    J = np.argmin(row, axis=0)                                               # the FIRST minimum: the shortest suffix, the largest start
    D = row[J, ar].astype(np.int64)
    hit = D <= k
    starts = np.where(hit, ends + 1 - J, 0).astype(np.uint64)
    starts[~hit] = NONE_START
    dist = np.where(hit, D, NONE_DIST).astype(np.uint8)
    words = np.zeros((E, 3), dtype=np.uint64)
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
    words[:, 2] |= np.where(hit, L << np.uint64(56), np.uint64(0))
    return starts, dist, words


def replay(ops, m, accepts, T, s, e):
    """True when the operations are an alignment of the pattern to T[s..e]: '=' on accepted symbols only, 'X' on others,
    m pattern symbols and e - s + 1 text symbols consumed.  Returns the number of edits."""
    i, p = 0, s
    for op in ops:
        if op in (EQ, SUB):
            assert i < m and p <= e and bool(accepts(i, np.asarray(T[p:p + 1]))[0]) == (op == EQ), (i, p, op)
            i, p = i + 1, p + 1
        elif op == INS:
            assert p <= e
            p += 1
        else:
            assert i < m
            i += 1
    assert i == m and p == e + 1, (i, p, m, e)
    return sum(1 for op in ops if op != EQ)


def test_the_oracle_against_edit_row_and_the_vector_oracle_is_the_definition():
    rng = np.random.default_rng(97)
    cases = 0
    for vals in ((65, 67, 71, 84), (0, 255), (7,)):
        for n, off in ((1, 0), (2, 0), (17, 0), (40, 0), (40, 13)):
            T = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]
            for m in (1, 2, 3, 8, 20, 33):
                P = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), m)]
                if m <= n - off and rng.integers(0, 2):
                    P = T[n - m:].copy()
                    if m > 2:
                        P = np.delete(P, m // 2)  # a pattern that needs an insertion
                sets = rng.integers(0, 1 << len(vals), len(P)).astype(np.uint8)
                for pat, accepts in ((P, byte_accepts(P)), (sets, set_accepts(sets, vals))):
                    mm = len(pat)
                    D = edit_row(mm, accepts, T, off)
                    ends = np.arange(off, n)
                    for k in (0, 2, 7):
                        starts, dist, words = align_many(mm, accepts, T, ends, k, off)
                        for x, e in enumerate(ends.tolist()):
                            one = align_one(mm, accepts, T, e, k, off)
                            if D[e - off] > k:  # the distances are edit_row's: the two oracles agree on what an occurrence is
                                assert one is None and starts[x] == NONE_START and dist[x] == NONE_DIST and not words[x].any()
                                continue
                            s, d, ops = one
                            assert d == D[e - off] and off <= s <= e + 1 and len(ops) <= mm + k
                            assert replay(ops, mm, accepts, T, s, e) == d
                            assert (int(starts[x]), int(dist[x]), words[x].tolist()) == (s, d, pack_ops(ops)), (vals, n, off, mm, k, e)
                            assert unpack_ops(words[x]) == ops
                        cases += 1
    assert cases == 3 * 5 * 6 * 2 * 3
    # the fixed choice among co-optimal alignments, by hand: P = AB against T = ...B: 'D' then '=' (rule 1 fails on A/B, rule 2 applies)
    T = np.frombuffer(b"CCB", dtype=np.uint8)
    P = np.frombuffer(b"AB", dtype=np.uint8)
    assert align_one(2, byte_accepts(P), T, 2, 1) == (2, 1, [DEL, EQ])
    # the largest start: P = AA on AAA ends at 2 with the match [1, 2], not [0, 2]
    T = np.frombuffer(b"AAA", dtype=np.uint8)
    assert align_one(2, byte_accepts(T[:2]), T, 2, 1) == (1, 0, [EQ, EQ])
    # k >= m: the empty match s = e + 1 with m 'D's when no symbol is accepted
    assert align_one(2, byte_accepts(np.frombuffer(b"GG", dtype=np.uint8)), T, 1, 2) == (2, 2, [DEL, DEL])


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
    # the edit calls no longer disclaim starts and alignments; the align calls say what THEY do not offer
    assert "start positions or alignments" not in raw
    assert "NOT offered: the longest start, all starts, all optimal alignments" in raw
    assert "opposite letters from SAM" in raw


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
    for name in ("palign_edit", "palign_sets_edit", "pfind_edit_align", "edit_cigar"):
        assert callable(getattr(smart_amd, name)), name
        assert getattr(smart_amd, name) is getattr(engine, name)


def test_sources_registry_has_the_unit_and_leaves_the_edit_unit_alone():
    assert [f for f in sources.UNITS["k_palign"] if f.startswith("k_")] == ["k_palign.hip"]
    for f in ("palign.hpp", "edit_align.hpp", "edit_step.hpp"):
        assert f in sources.UNITS["k_palign"], f
    assert sources.KERNEL_UNIT["planes_edit_align"] == "k_palign"
    assert sources.kernel_sha256("planes_edit_align") == sources.unit_sha256("k_palign") != sources.unit_sha256("k_pedit")
    assert sources.UNITS["k_pedit"] == ("k_pedit.hip", "pedit.hpp", "pedit_host.hpp", "edit_step.hpp", "planes.hpp")
    makefile = open(os.path.join(sources.CSRC, "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bk_palign\b", makefile, flags=re.M)


def test_documents_name_every_symbol():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in list(SYMBOLS) + ["palign_edit", "palign_sets_edit", "pfind_edit_align", "edit_cigar"]:
        assert n in doc, n
    assert "smartgpu_palign_edit64" in open(os.path.join(ROOT, "README.md")).read()
    assert "planes_edit_align" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(rc, says):
    assert rc == ERR_ARG, rc
    msg = engine.lib().smartgpu_last_error().decode()
    assert says in msg, (says, msg)


@pytest.mark.parametrize("kind", ["", "_sets"])
def test_refusals_that_need_no_device(kind):
    """Without a device there is no handle: every call passes a NULL text, so each is decided before the first HIP call, for
    the reason its line states, and writes nothing.  (An end outside a REAL range is refused in tests/test_packed_align_gpu.py.)"""
    f = getattr(engine.lib(), "smartgpu_palign%s_edit64" % kind)
    P = np.full(100, 1, dtype=np.uint8)
    ends = np.arange(8, dtype=np.uint64)
    starts = np.full(8, 77, dtype=np.uint64)
    dist = np.full(8, 7, dtype=np.uint8)
    ops = np.full(24, 5, dtype=np.uint64)
    call = lambda p, m, k, e, cnt, s: f(p, m, k, None, 0, 100, e, cnt, s, dist.ctypes.data, ops.ctypes.data)  # noqa: E731
    _refused(call(None, 4, 1, ends.ctypes.data, 8, starts.ctypes.data), "sets is NULL" if kind else "P is NULL")
    _refused(call(P.ctypes.data, 0, 1, ends.ctypes.data, 8, starts.ctypes.data), "length 0 outside [1,64]")
    _refused(call(P.ctypes.data, 65, 1, ends.ctypes.data, 8, starts.ctypes.data), "length 65 outside [1,64]")
    _refused(call(P.ctypes.data, 4, 8, ends.ctypes.data, 8, starts.ctypes.data), "k = 8 ")
    _refused(call(P.ctypes.data, 4, 1, None, 8, starts.ctypes.data), "ends NULL")
    _refused(call(P.ctypes.data, 4, 1, ends.ctypes.data, 8, None), "starts NULL")
    _refused(call(P.ctypes.data, 4, 1, ends.ctypes.data, 8, starts.ctypes.data), "handle is NULL")
    _refused(call(P.ctypes.data, 4, 1, None, 0, None), "handle is NULL")  # count == 0 excuses the NULL lists, not the NULL text
    assert (starts == 77).all() and (dist == 7).all() and (ops == 5).all()


# ---- edit_cigar --------------------------------------------------------------------------------------------------------

def test_edit_cigar_on_hand_written_words():
    # 12 '=', 1 'X', 3 '=', 1 'D', 4 '=': 21 operations in the first word
    ops = [EQ] * 12 + [SUB] + [EQ] * 3 + [DEL] + [EQ] * 4
    w0 = (1 << 2 * 12) | (3 << 2 * 16)
    assert pack_ops(ops) == [w0, 0, 21 << 56]
    assert smart_amd.edit_cigar(np.array([w0, 0, 21 << 56], dtype=np.uint64)) == "12=1X3=1D4="
    assert smart_amd.edit_cigar([w0, 0, 21 << 56], sam=True) == "12=1X3=1I4="
    # operations in all three words: 30 '=', 4 'I' across the first seam, 29 '=', 2 'D' across the second, 3 'X': 68
    ops = [EQ] * 30 + [INS] * 4 + [EQ] * 29 + [DEL] * 2 + [SUB] * 3
    words = pack_ops(ops)
    assert words[0] >> 60 == 0b1010 and words[1] & 0xF == 0b1010 and words[1] >> 62 == DEL and words[2] & 0xFF == 0b01010111
    assert smart_amd.edit_cigar(np.array(words, dtype=np.uint64)) == "30=4I29=2D3X"
    assert smart_amd.edit_cigar(np.array(words, dtype=np.uint64), sam=True) == "30=4D29=2I3X"
    # the sentinel of a non-occurrence and the longest alignment
    assert smart_amd.edit_cigar(np.zeros(3, dtype=np.uint64)) == ""
    assert smart_amd.edit_cigar(np.array(pack_ops([DEL] * 71), dtype=np.uint64)) == "71D"
    with pytest.raises(ValueError):
        smart_amd.edit_cigar([0, 0])


# ---- the shared header on the CPU ----------------------------------------------------------------------------------------

def test_distance_step_cells_and_traceback_on_the_host(tmp_path):
    """tests/packed_align_check.cpp, compiled with AddressSanitizer and UBSan, run as a child process: edit_align.hpp fed as
    the kernel feeds it, against a scalar DP of the suffix distances written out in the program — start, distance and every
    operation, and the packing (length byte, unused bits zero)."""
    exe = tmp_path / "packed_align_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "smart_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "packed_align_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    summary = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert summary, r.stdout[-2000:] + r.stderr[-4000:]
    cases, failures = map(int, summary.groups())
    # per length: 4 alphabets x 2 kinds of pattern x 4 values of k x (every end of the text + the walks clipped at off),
    # + both kinds of end seen + the all-equal case + the end with D(e) > k; 4 lengths on one dword, 7 on two
    assert r.returncode == 0 and failures == 0 and cases == (4 + 7) * (4 * 2 * 4 * 2 + 3), r.stdout[-4000:] + r.stderr[-2000:]


def test_the_unit_holds_the_kernels_without_scratch_and_static_lds():
    """planes_edit_align for one and two planes, one and two dwords, with and without the traceback: eight kernels of the
    k_palign code object, each with ScratchSize 0 and no static LDS (-Rpass-analysis=kernel-resource-usage, as
    tests/test_packed_edit.py reads it; the traceback's LDS is dynamic and does not show here)."""
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", os.path.join(sources.CSRC, "k_palign.hip")]
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
    assert len([k for k in usage if "planes_edit_align" in k]) == 8, sorted(usage)
    for planes in (1, 2):
        for words in (1, 2):
            for ops in (0, 1):
                mine = [k for k in usage if re.search(r"planes_edit_alignILi%dELi%dELb%dEE" % (planes, words, ops), k)]
                assert len(mine) == 1, (planes, words, ops, sorted(usage))
                assert usage[mine[0]] == {"scratch": 0, "lds": 0}, (mine[0], usage[mine[0]])
    # the dynamic LDS the launcher asks for stays within 64 KB: the constants of the kernel's geometry, restated
    text = open(os.path.join(sources.CSRC, "k_palign.hip")).read()
    assert re.search(r"kLanes = \(WORDS == 2 && OPS\) \? 32 : 64;", text) and re.search(r"kCols = WORDS == 2 \? 72 : 40;", text)
    assert max(40 * 2 * 64 * 4, 72 * 4 * 32 * 4) <= 64 * 1024
