"""Mismatches on BYTE texts on the GPU (smartgpu_search_mis64, smartgpu_find_mis64 and their classes forms; text_mis_scan and
text_mis_find of k_tmis.hip) against the definition: by_definition of tests/test_packed_mis_gpu.py, generalised to an
`accepts` predicate so that it reads classes as well.  Every comparison is exact equality, of the count, the start positions
AND the distances.

Texts have at most 2^20 + 3 bytes.  A window's distance does not depend on k, so every (alphabet, n, m) builds ONE text, planted
with copies of the pattern that carry 0 .. 8 substitutions (0 .. k + 1 for every k of the grid), uploads it once, runs the
definition once at k = 8 and checks the calls at every k against its entries with distance <= k."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402

import smart_amd  # noqa: E402
from smart_amd import (PackedText, Text, byte_classes, engine, find, find_edit, find_mis, find_mis_classes, pfind_mis,  # noqa: E402
                       search_mis, search_mis_classes)

from tiled_oracle import edited  # noqa: E402

ERR_ARG, ERR_NOMEM = -3, -5
RUN, WAVE_RUN, WG_RUN = 128, 8192, 32768  # what a lane, a wave and a workgroup own per trip (k_tmis.hip)
ALPHABETS = {
    "two": (0, 255),
    "acgt": (65, 67, 71, 84),
    "amino": tuple(b"ACDEFGHIKLMNPQRSTVWY"),
    "all256": tuple(range(256)),
    "english": None,
}
MS = (1, 2, 31, 32, 33, 63, 64)
KS = (0, 1, 3, 7)
NS = (1, 2, 127, 128, 129, 8191, 8192, 8193, 32769, 2**20 + 3)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


@functools.lru_cache(maxsize=None)
def english():
    T = np.fromfile(os.path.join(ROOT, "tests", "golden", "english_excerpt.txt"), dtype=np.uint8)
    T.setflags(write=False)
    return T


def draw(name, n, rng):
    """(n bytes of the alphabet, the values `edited` substitutes)."""
    if name == "english":
        E = english()
        reps = -(-(n + 1000) // len(E))
        return np.tile(E, reps)[777:777 + n].copy(), tuple(np.unique(E).tolist())
    vals = ALPHABETS[name]
    return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)], vals


@contextlib.contextmanager
def uploaded(T):
    text = Text.upload(T)
    try:
        yield text
    finally:
        text.free()


# ---- the definition ----------------------------------------------------------------------------------------------------

def byte_accepts(P):
    return lambda j, B: B == P[j]


def class_accepts(classes):
    return lambda j, B: ((classes[j][B >> 3] >> (B & 7)) & 1).astype(bool)


def by_definition(m, accepts, T, k, off=0, n=None):
    """(ascending start positions relative to byte 0 as uint64, their distances as uint8) in [off, off + n - m]: the distance
    of start s is the number of j < m whose position does not accept T[s + j].  A progressive filter — the candidates' running
    mismatch counts, candidates dropped once they are over k."""
    n = len(T) - off if n is None else n
    if m > n:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    s = np.arange(off, off + n - m + 1, dtype=np.int64)
    d = np.zeros(len(s), dtype=np.int32)
    for j in range(m):
        d += ~accepts(j, T[s + j])
        keep = d <= k
        if not keep.all():
            s, d = s[keep], d[keep]
            if len(s) == 0:
                break
    return s.astype(np.uint64), d.astype(np.uint8)


def within(entries, k):
    pos, dist = entries
    keep = dist <= k
    return pos[keep], dist[keep]


def first_difference(a, b):
    at = int(np.flatnonzero(a != b)[0])
    return at, int(a[at]), int(b[at])


def check(text, want, k, off, n, count, find, what=()):
    """The count call and the find call at k against the definition's (positions, distances)."""
    wpos, wdist = want
    got = count(text, k, off, n)
    assert got == len(wpos), (what, k, off, n, got, len(wpos))
    pos, dist = find(text, k, off, n, max(len(wpos), 1))
    assert pos.dtype == np.uint64 and dist.dtype == np.uint8 and len(pos) == len(dist) == len(wpos), (what, k, off, n, len(pos), len(wpos))
    assert np.array_equal(pos, wpos), (what, k, off, n, first_difference(pos, wpos))
    assert np.array_equal(dist, wdist), (what, k, off, n, first_difference(dist, wdist))
    return len(wpos)


def check_bytes(text, T, P, k, off=0, n=None, want=None):
    n = len(T) - off if n is None else n
    want = by_definition(len(P), byte_accepts(P), T, k, off, n) if want is None else want
    return check(text, want, k, off, n, lambda t, k, off, n: search_mis(P, t, k, off=off, n=n),
                 lambda t, k, off, n, cap: find_mis(P, t, k, off=off, n=n, cap=cap), ("bytes", len(P)))


def check_classes(text, T, classes, k, off=0, n=None, want=None):
    n = len(T) - off if n is None else n
    want = by_definition(len(classes), class_accepts(classes), T, k, off, n) if want is None else want
    return check(text, want, k, off, n, lambda t, k, off, n: search_mis_classes(classes, t, k, off=off, n=n),
                 lambda t, k, off, n, cap: find_mis_classes(classes, t, k, off=off, n=n, cap=cap), ("classes", len(classes)))


def plant(T, P, vals, ds, rng):
    """Copies of P with d substitutions for d in ds, spread over T where T has the room; returns the d that went in."""
    n, m, done = len(T), len(P), []
    for t, d in enumerate(ds):
        try:
            W = edited(P, d, rng, vals, False) if d else P.copy()
        except ValueError:  # the pattern has fewer than d places to substitute
            continue
        a = (t + 1) * n // (len(ds) + 2)
        if n < (len(ds) + 2) * (m + 12) or a + m > n:
            continue
        T[a:a + m] = W
        done.append(d)
    return done


# ---- alphabets x lengths x k x n -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ALPHABETS))
def test_alphabets_lengths_and_k(name):
    """Every m, k and n of the grid on one alphabet.  The pattern is cut from the text (drawn from the alphabet where the text
    is shorter) and copies with 0 .. 8 substitutions are planted where the text has the room: on the largest text every k of
    the grid has occurrences at distance exactly k and near-misses at k + 1 (m >= 31)."""
    rng = np.random.default_rng(1500 + list(ALPHABETS).index(name))
    cases = hits = 0
    for n in NS:
        for m in MS:
            T, vals = draw(name, n, rng)
            if n >= m:
                a = int(rng.integers(0, n - m + 1))
                P = T[a:a + m].copy()
            else:
                P = draw(name, m, rng)[0]
            planted = plant(T, P, vals, range(9), rng)
            all8 = by_definition(m, byte_accepts(P), T, 8)
            if n == NS[-1] and m >= 31:
                assert planted == list(range(9)) and set(range(9)) <= set(all8[1].tolist()), (name, m, planted)  # (the inputs)
            with uploaded(T) as text:
                for k in KS:
                    hits += check_bytes(text, T, P, k, want=within(all8, k))
                    cases += 1
    assert cases == len(NS) * len(MS) * len(KS) and hits > cases


# ---- seams ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [2, 20, 33, 64])
def test_copies_at_the_seams_of_lanes_waves_and_workgroups(m):
    """Copies of the pattern with min(k, 1) substitutions (none at m = 2) that END at r - 1, r or r + 1, or BEGIN there, for
    r = 128 (two lanes), 8192 (two waves) and 32768 (two workgroups), over 256 values."""
    rng = np.random.default_rng(1700 + m)
    vals = tuple(range(256))
    n = WG_RUN + WAVE_RUN + 301
    for k in KS:
        for edge in ("end", "begin"):
            for by in (-1, 0, 1):
                T = rng.integers(0, 256, n).astype(np.uint8)
                P = rng.integers(0, 256, m).astype(np.uint8)
                d = min(k, 1) if m > 2 else 0
                wanted = []
                for r in (RUN, WAVE_RUN, WG_RUN):
                    a = r + by if edge == "begin" else r + by - m + 1
                    T[a:a + m] = edited(P, d, rng, vals, False) if d else P
                    wanted.append(a)
                want = by_definition(m, byte_accepts(P), T, k)
                assert set(wanted) <= set(want[0].tolist())  # (the inputs)
                with uploaded(T) as text:
                    assert check_bytes(text, T, P, k, want=want) >= 3


def test_a_window_that_ends_on_every_byte_of_two_runs_and_a_span_seam():
    """The same copy slid over every end position of [8192 - 130, 8192 + 130): no residue of the run or of the dword is special."""
    rng = np.random.default_rng(1750)
    m, k = 33, 3
    P = rng.integers(0, 256, m).astype(np.uint8)
    n = WAVE_RUN + 1000
    base = rng.integers(0, 256, n).astype(np.uint8)
    W = edited(P, k, rng, tuple(range(256)), False)
    for e in range(WAVE_RUN - 130, WAVE_RUN + 130, 7):
        T = base.copy()
        T[e - m + 1:e + 1] = W
        with uploaded(T) as text:
            pos, dist = find_mis(P, text, k)
            assert pos.tolist() == [e - m + 1] and dist.tolist() == [k], (e, pos, dist)
            assert search_mis(P, text, k - 1) == 0


# ---- ranges --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [1, 2, 127, 128, 129, 8191, 8193, 40001])
def test_ranges_hold_whole_windows_only(off):
    """"cut": an exact copy lies across `off`, its first bytes BEFORE the range, and another across off + n — neither is an
    occurrence of the range, though both are occurrences of the text.  "exact": a copy BEGINS at the range's first byte and one
    ENDS with its last byte — both are.  Ranges that start and end mid-dword and mid-run, one whose end is one short of a run,
    one that ends with the text."""
    rng = np.random.default_rng(1900 + off)
    n_text = 40001 + 3 * WAVE_RUN + 77
    one_short = (off + 2 * WAVE_RUN) // RUN * RUN + RUN - 1 - off
    assert (off + one_short + 1) % RUN == 0
    for m, k in ((20, 3), (64, 7), (2, 0)):
        for n in (n_text - off - 1000 - 37, one_short, n_text - off):
            for edge in ("cut", "exact"):
                T = rng.integers(0, 256, n_text).astype(np.uint8)
                P = rng.integers(0, 256, m).astype(np.uint8)
                h = min(2, m - 1, off)
                starts = (off - h, off + n - m + h) if edge == "cut" else (off, off + n - m)
                for a in starts + (off + 5000,):
                    if a + m <= n_text:
                        T[a:a + m] = P
                want = by_definition(m, byte_accepts(P), T, k, off, n)
                if m > 2:  # (the inputs) over 256 values nothing but the copies is near
                    assert want[0].tolist() == ([off + 5000] if edge == "cut" else [off, off + 5000, off + n - m])
                    whole = by_definition(m, byte_accepts(P), T, k)[0].tolist()
                    assert all(a in whole for a in starts if a + m <= n_text)  # and the cut copies are occurrences of the text
                with uploaded(T) as text:
                    assert check_bytes(text, T, P, k, off, n, want=want) >= 1


def test_m_greater_than_n_is_count_zero():
    T = np.frombuffer(b"abcabcabcabc", dtype=np.uint8)
    with uploaded(T) as text:
        for m, off, n in ((5, 0, 4), (64, 3, 9), (2, 12, 0), (1, 5, 0)):
            P = np.resize(T, m)
            assert search_mis(P, text, 7, off=off, n=n) == 0
            pos, dist = find_mis(P, text, 7, off=off, n=n)
            assert len(pos) == 0 and len(dist) == 0
        assert search_mis(T[:5], text, 0, off=0, n=5) == 1  # m == n: one window


# ---- degenerate shapes -----------------------------------------------------------------------------------------------------

def test_k_at_least_m_reports_every_start_with_its_distance():
    rng = np.random.default_rng(2000)
    T = np.asarray(ALPHABETS["acgt"], dtype=np.uint8)[rng.integers(0, 4, 20011)]
    with uploaded(T) as text:
        for m, k in ((1, 1), (1, 7), (2, 3), (7, 7), (3, 7)):
            P = np.asarray(ALPHABETS["acgt"], dtype=np.uint8)[rng.integers(0, 4, m)]
            for off, n in ((0, len(T)), (131, 9000)):
                want = by_definition(m, byte_accepts(P), T, k, off, n)
                assert len(want[0]) == n - m + 1 and len(set(want[1].tolist())) > 1  # (the inputs) every start, several distances
                check_bytes(text, T, P, k, off, n, want=want)


def test_a_pattern_byte_the_text_does_not_hold():
    """It is a mismatch in every window: nothing at k = 0, the planted copies one further away."""
    rng = np.random.default_rng(2100)
    T = np.asarray(ALPHABETS["acgt"], dtype=np.uint8)[rng.integers(0, 4, 50021)]
    for m in (20, 40):
        P = T[777:777 + m].copy()
        T[30000:30000 + m] = edited(P, 2, rng, ALPHABETS["acgt"], False)
        P[m // 2] = ord("N")
        assert ord("N") not in T
        with uploaded(T) as text:
            assert search_mis(P, text, 0) == 0
            for k in (1, 3):
                want = by_definition(m, byte_accepts(P), T, k)
                assert 777 in want[0].tolist() and (k < 3 or 30000 in want[0].tolist()) and want[1].min() >= 1
                check_bytes(text, T, P, k, want=want)


# ---- classes -------------------------------------------------------------------------------------------------------------

def test_singleton_classes_equal_the_byte_calls():
    rng = np.random.default_rng(2200)
    T, vals = draw("amino", 70001, rng)
    for m in (1, 20, 33, 64):
        P = T[4000:4000 + m].copy()
        plant(T, P, vals, range(9), rng)
        with uploaded(T) as text:
            for k in KS:
                want = by_definition(m, byte_accepts(P), T, k)
                check_classes(text, T, byte_classes(P), k, want=want)
                check_bytes(text, T, P, k, want=want)


def test_ignore_case_on_english():
    T = np.tile(english(), 3)[:150001].copy()
    for word, k in ((b"the", 0), (b"Which", 1), (b"government", 2)):
        P = np.frombuffer(word, dtype=np.uint8)
        a = 50000 + 1000 * k
        T[a:a + len(P)] = np.frombuffer(word.upper(), dtype=np.uint8)  # a copy in the other case
        classes = byte_classes(P, ignore_case=True)
        want = by_definition(len(P), class_accepts(classes), T, k)
        folded = np.frombuffer(bytes(T).lower(), dtype=np.uint8)
        low = by_definition(len(P), byte_accepts(np.frombuffer(word.lower(), dtype=np.uint8)), folded, k)
        assert np.array_equal(want[0], low[0]) and np.array_equal(want[1], low[1]) and a in want[0].tolist()  # (the inputs)
        with uploaded(T) as text:
            n_folded = check_classes(text, T, classes, k, want=want)
            assert n_folded > search_mis(P, text, k)  # the byte call misses the other case


def test_an_empty_row_and_a_full_row():
    """An empty row is a mismatch in every window — nothing at k = 0, the exact copies at distance 1 —, a full row never is:
    the copies whose only substitution lies under it are at distance 0."""
    rng = np.random.default_rng(2300)
    for m in (20, 33):
        T = rng.integers(0, 256, 60013).astype(np.uint8)
        P = rng.integers(0, 256, m).astype(np.uint8)
        T[1000:1000 + m] = P
        W = P.copy()
        W[5] ^= 0x55
        T[41000:41000 + m] = W
        classes = byte_classes(P)
        classes[5, :] = 0xFF
        with uploaded(T) as text:
            want = by_definition(m, class_accepts(classes), T, 0)
            assert want[0].tolist() == [1000, 41000] and want[1].tolist() == [0, 0]
            check_classes(text, T, classes, 0, want=want)
            classes[m - 2, :] = 0
            assert search_mis_classes(classes, text, 0) == 0
            for k in (1, 3):
                want = by_definition(m, class_accepts(classes), T, k)
                assert want[0].tolist() == [1000, 41000] and want[1].tolist() == [1, 1]
                check_classes(text, T, classes, k, want=want, off=0)
            check_classes(text, T, classes, 3, off=999, n=45000)


@pytest.mark.parametrize("m", [1, 32, 33, 64])
def test_full_rows_everywhere_give_every_start_at_distance_zero(m):
    rng = np.random.default_rng(2400 + m)
    T = rng.integers(0, 256, WG_RUN + 4099).astype(np.uint8)
    classes = np.full((m, 32), 0xFF, dtype=np.uint8)
    with uploaded(T) as text:
        for off, n in ((0, len(T)), (77, WG_RUN + 130)):
            for k in (0, 7):
                assert search_mis_classes(classes, text, k, off=off, n=n) == n - m + 1
                pos, dist = find_mis_classes(classes, text, k, off=off, n=n)
                assert np.array_equal(pos, np.arange(off, off + n - m + 1, dtype=np.uint64)) and not dist.any()


# ---- relations to the other calls ------------------------------------------------------------------------------------------

def test_k_zero_equals_find():
    rng = np.random.default_rng(2500)
    for name in ("two", "english"):
        T, _ = draw(name, 300007, rng)
        with uploaded(T) as text:
            for m in (1, 2, 8, 32, 33, 64):
                P = T[123457:123457 + m].copy()
                want, cnt = find(P, text)
                pos, dist = find_mis(P, text, 0, cap=max(cnt, 1))
                assert cnt == len(pos) >= 1 and np.array_equal(pos, want) and not dist.any(), (name, m)
                assert search_mis(P, text, 0) == cnt


def test_acgt_equals_pfind_mis_on_the_same_bytes_packed():
    rng = np.random.default_rng(2600)
    T, vals = draw("acgt", 2**18 + 77, rng)
    with uploaded(T) as text:
        pt = PackedText.pack(text)
        try:
            for m in (8, 20, 32, 33, 64):
                P = T[5555:5555 + m].copy()
                for k in KS:
                    for off, n in ((0, len(T)), (1001, 2**17 + 5)):
                        ppos, pdist, pcnt = pfind_mis(P, pt, k, off=off, n=n)
                        pos, dist = find_mis(P, text, k, off=off, n=n)
                        assert pcnt == len(pos) >= (off == 0) and np.array_equal(pos, ppos) and np.array_equal(dist, pdist), (m, k, off)
        finally:
            pt.free()


def test_every_occurrence_ends_where_find_edit_reports_an_end():
    """At equal k a Hamming occurrence is an edit occurrence: s + m - 1 is among find_edit's ends, with a distance at least the
    edit distance; the edit call has ends that are no Hamming occurrence (a strict superset once k >= 1)."""
    rng = np.random.default_rng(2700)
    T, vals = draw("amino", 200003, rng)
    for m in (12, 40):
        P = T[9000:9000 + m].copy()
        plant(T, P, vals, range(9), rng)
        T[150000:150000 + m - 1] = np.delete(P, m // 2)  # one deletion: within one edit, m / 2 substitutions away
        with uploaded(T) as text:
            for k in (1, 3, 7):
                pos, dist = find_mis(P, text, k)
                ends, edist = find_edit(P, text, k)
                at = np.searchsorted(ends, pos + np.uint64(m - 1))
                assert len(pos) >= 3 and (at < len(ends)).all() and np.array_equal(ends[at], pos + np.uint64(m - 1)), (m, k)
                assert (edist[at] <= dist).all()
                assert len(ends) > len(pos) and 150000 + m - 2 in ends.tolist()


# ---- cap, count, refusals on a real text -----------------------------------------------------------------------------------

def test_cap_exact_one_short_and_zero():
    rng = np.random.default_rng(2800)
    T, vals = draw("acgt", 100003, rng)
    m, k = 12, 3
    P = T[100:100 + m].copy()
    want = by_definition(m, byte_accepts(P), T, k)
    total = len(want[0])
    assert total > 20
    L = engine.lib()
    with uploaded(T) as text:
        for kind, pat in (("", P), ("_classes", byte_classes(P))):
            f = getattr(L, "smartgpu_find_mis%s64" % kind)
            pos = np.full(total + 2, 0xABABABABABABABAB, dtype=np.uint64)
            dist = np.full(total + 2, 0xCD, dtype=np.uint8)
            c = ctypes.c_uint64(0)
            assert f(pat.ctypes.data, m, k, text._h, 0, len(T), pos.ctypes.data, dist.ctypes.data, total, ctypes.byref(c)) == 0
            assert c.value == total and np.array_equal(pos[:total], want[0]) and np.array_equal(dist[:total], want[1])
            assert (pos[total:] == 0xABABABABABABABAB).all() and (dist[total:] == 0xCD).all()  # nothing behind cap is touched
            c = ctypes.c_uint64(0)
            assert f(pat.ctypes.data, m, k, text._h, 0, len(T), pos.ctypes.data, dist.ctypes.data, total - 1, ctypes.byref(c)) == ERR_NOMEM
            assert c.value == total and str(total) in L.smartgpu_last_error().decode()
            c = ctypes.c_uint64(0)
            assert f(pat.ctypes.data, m, k, text._h, 0, len(T), None, None, 0, ctypes.byref(c)) == (0 if total == 0 else ERR_NOMEM)
            assert c.value == total  # cap == 0 with NULL buffers: a count call
            c = ctypes.c_uint64(0)
            assert f(pat.ctypes.data, m, k, text._h, 0, len(T), pos.ctypes.data, None, total, ctypes.byref(c)) == 0  # mismatches may be NULL
            assert c.value == total and np.array_equal(pos[:total], want[0])


def test_refusals_on_a_real_text_write_nothing():
    T = np.arange(1000, dtype=np.uint64).astype(np.uint8)
    L = engine.lib()
    P = T[:8].copy()
    with uploaded(T) as text:
        c = ctypes.c_uint64(77)
        pre, run = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
        for off, n in ((1001, 0), (0, 1001), (990, 11), (2**63, 2**63)):
            assert L.smartgpu_search_mis64(P.ctypes.data, 8, 1, text._h, off, n, ctypes.byref(c), ctypes.byref(pre), ctypes.byref(run)) == ERR_ARG
            assert "search_mis64: range" in L.smartgpu_last_error().decode()
        assert L.smartgpu_search_mis64(P.ctypes.data, 8, 1, text._h, 0, 1000, None, ctypes.byref(pre), ctypes.byref(run)) == ERR_ARG
        assert "search_mis64: count must not be NULL" in L.smartgpu_last_error().decode()
        assert L.smartgpu_find_mis64(P.ctypes.data, 8, 1, text._h, 0, 1000, None, None, 0, None) == ERR_ARG
        assert "find_mis64: count must not be NULL" in L.smartgpu_last_error().decode()
        assert c.value == 77 and pre.value == -1.0 and run.value == -2.0
        # and the times of a call that ran are written
        assert L.smartgpu_search_mis64(P.ctypes.data, 8, 1, text._h, 0, 1000, ctypes.byref(c), ctypes.byref(pre), ctypes.byref(run)) == 0
        assert c.value >= 1 and pre.value >= 0.0 and run.value > 0.0
