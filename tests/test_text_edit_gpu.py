"""Edit distance on BYTE texts on the GPU (smartgpu_search_edit64, smartgpu_find_edit64 and their classes forms; text_edit_scan
and text_edit_find of k_tedit.hip) against the by-definition oracle of tests/test_packed_edit.py (edit_row / edit_occurrences:
Sellers' programme on the range alone).  Every comparison is exact equality, of the count, the ends AND the distances.

Texts have at most 2^20 + 3 bytes.  The oracle's row D(e) does not depend on k, so every (alphabet, n, m) builds ONE text,
planted with copies of the pattern that carry 0 .. 8 edits (0 .. k + 1 for every k of the grid), uploads it once, runs the
oracle once and checks the calls at every k against that row: the whole grid alphabets x m x k x n runs, and the oracle's
226 passes over the largest text stay at a couple of seconds per alphabet."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402

import smart_amd  # noqa: E402
from smart_amd import (PackedText, Plan, SmartGpuError, Text, byte_classes, engine, find, find_edit, find_edit_classes, pfind_edit,  # noqa: E402
                       search_edit, search_edit_classes)

from test_packed_edit import byte_accepts, edit_occurrences, edit_row  # noqa: E402
from tiled_oracle import edited  # noqa: E402

ERR_NOMEM = -5
RUN, WAVE_RUN, WG_RUN = 128, 8192, 32768  # what a lane, a wave and a workgroup own per trip (k_tedit.hip)
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
    """(n bytes of the alphabet, the values `edited` substitutes and inserts)."""
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


def class_accepts(classes):
    """The oracle's accepts(i, R) of an (m, 32) classes array."""
    return lambda i, R: ((classes[i][R >> 3] >> (R & 7)) & 1).astype(bool)


def plant(T, P, vals, ds, rng):
    """Copies of P with d edits of mixed kinds for d in ds, spread over T where T has the room; returns how many went in."""
    n, m, done = len(T), len(P), 0
    for t, d in enumerate(ds):
        try:
            W = edited(P, d, rng, vals, True) if d else P.copy()
        except ValueError:  # the pattern has fewer than d places to edit
            continue
        a = (t + 1) * n // (len(ds) + 2)
        if n < (len(ds) + 2) * (m + 12) or a + len(W) > n:
            continue
        T[a:a + len(W)] = W
        done += 1
    return done


def check(text, want_row, k, off=0, n=None, count=None, find=None, what=()):
    """The count call and the find call at k against the oracle's row over the range (want_row[i] = D(off + i))."""
    n = len(want_row) if n is None else n
    at = np.flatnonzero(want_row <= k)
    wends, wdist = (at + off).astype(np.uint64), want_row[at].astype(np.uint8)
    got = count(text, k, off, n)
    assert got == len(wends), (what, k, off, n, got, len(wends))
    ends, dist = find(text, k, off, n, max(len(wends), 1))
    assert ends.dtype == np.uint64 and dist.dtype == np.uint8 and len(ends) == len(dist) == len(wends), (what, k, off, n, len(ends), len(wends))
    assert np.array_equal(ends, wends), (what, k, off, n, first_difference(ends, wends))
    assert np.array_equal(dist, wdist), (what, k, off, n, first_difference(dist, wdist))
    return len(wends)


def check_bytes(text, T, P, k, off=0, n=None, row=None):
    n = len(T) - off if n is None else n
    row = edit_row(len(P), byte_accepts(P), T, off, n) if row is None else row
    return check(text, row, k, off, n, lambda t, k, off, n: search_edit(P, t, k, off=off, n=n),
                 lambda t, k, off, n, cap: find_edit(P, t, k, off=off, n=n, cap=cap), ("bytes", len(P)))


def first_difference(a, b):
    at = int(np.flatnonzero(a != b)[0])
    return at, int(a[at]), int(b[at])


# ---- alphabets x lengths x k -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ALPHABETS))
def test_alphabets_lengths_and_k(name):
    """Every m, k and n of the grid on one alphabet.  The pattern is cut from the text (drawn from the alphabet where the text
    is shorter) and copies with 0 .. 8 edits of mixed kinds are planted where the text has the room."""
    rng = np.random.default_rng(500 + list(ALPHABETS).index(name))
    cases = hits = planted = 0
    for n in NS:
        for m in MS:
            T, vals = draw(name, n, rng)
            if n >= m:
                a = int(rng.integers(0, n - m + 1))
                P = T[a:a + m].copy()
            else:
                P = draw(name, m, rng)[0]
            planted += plant(T, P, vals, range(9), rng)
            row = edit_row(m, byte_accepts(P), T)
            with uploaded(T) as text:
                for k in KS:
                    hits += check_bytes(text, T, P, k, row=row)
                    cases += 1
    assert cases == len(NS) * len(MS) * len(KS) and planted >= 9 * 5 * 3 and hits > cases


# ---- seams ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [20, 33, 64])
def test_copies_at_the_seams_of_lanes_waves_and_workgroups(m):
    """Copies of the pattern with min(k, 1) edits that END at r - 1, r and r + 1, and copies that BEGIN exactly m + k before r,
    for r = 128 (two lanes), 8192 (two waves) and 32768 (two workgroups), over 256 values: nothing but the copies is near."""
    rng = np.random.default_rng(700 + m)
    vals = tuple(range(256))
    n = WG_RUN + WAVE_RUN + 301
    for k in KS:
        for where in ("end-1", "end", "end+1", "begin"):
            T = np.asarray(vals, dtype=np.uint8)[rng.integers(0, 256, n)]
            P = np.asarray(vals, dtype=np.uint8)[rng.integers(0, 256, m)]
            wanted = []
            for r in (RUN, WAVE_RUN, WG_RUN):
                W = edited(P, min(k, 1), rng, vals, True)
                if where == "begin":
                    a = r - (m + k)
                else:
                    a = r + {"end-1": -1, "end": 0, "end+1": 1}[where] - len(W) + 1
                T[a:a + len(W)] = W
                wanted.append(a + len(W) - 1)
            row = edit_row(m, byte_accepts(P), T)
            assert all(row[e] == min(k, 1) for e in wanted), (m, k, where)  # (the inputs) the copies are what the oracle finds
            with uploaded(T) as text:
                assert check_bytes(text, T, P, k, row=row) >= 3


# ---- ranges --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [1, 127, 128, 129, 8191, 8193, 40001])
def test_ranges_read_nothing_before_their_first_byte(off):
    """A copy of the pattern lies across `off`, its first h bytes just BEFORE the range: on the range alone its end is h edits
    away (h = 2) or no occurrence at all (h = m / 2) — a kernel that reads a distance out of bytes before the range reports 0.
    Once with a range that ends mid-run, once with one that ends with the text."""
    rng = np.random.default_rng(900 + off)
    m, k = 20, 3
    n_text = 40001 + 3 * WAVE_RUN + 77
    for h in (2, m // 2):
        T = rng.integers(0, 256, n_text).astype(np.uint8)
        P = rng.integers(0, 256, m).astype(np.uint8)
        T[off - min(h, off):off - min(h, off) + m] = P
        T[off + 5000:off + 5000 + m] = P
        with uploaded(T) as text:
            for n in (n_text - off - 1000 - 37, n_text - off):
                assert (off + n) % RUN != 0 or off + n == n_text
                row = edit_row(m, byte_accepts(P), T, off, n)
                hh = min(h, off)
                e = m - 1 - hh  # (the inputs) the copy's end, relative to off: hh edits away on the range alone, none on the text
                assert (row[e] == hh if hh <= k else row[e] > k) and edit_row(m, byte_accepts(P), T)[e + off] == 0
                assert check_bytes(text, T, P, k, off, n, row=row) >= 1


# ---- degenerate shapes -----------------------------------------------------------------------------------------------------

def test_k_at_least_m_reports_every_end_with_its_distance():
    rng = np.random.default_rng(1100)
    n = 3 * WAVE_RUN + 5
    T = np.asarray(tuple(b"ACDEFGHIKLMNPQRSTVWY"), dtype=np.uint8)[rng.integers(0, 20, n)]
    for m, k in ((3, 3), (5, 7), (1, 1)):
        P = T[100:100 + m].copy()
        with uploaded(T) as text:
            assert check_bytes(text, T, P, k) == n


def test_ranges_shorter_than_the_pattern_and_foreign_bytes():
    P = np.frombuffer(b"ACGTTGCA", dtype=np.uint8)
    T = np.frombuffer(b"TTACGTTGG", dtype=np.uint8)
    with uploaded(T) as text:
        # m > n with n + k >= m: the range "ACGTT" is P without its last three bytes
        assert check_bytes(text, T, P, 3, 2, 5) == 1
        assert check_bytes(text, T, P, 7, 2, 5) == 5
        # n + k < m: nothing, without a launch
        assert search_edit(P, text, 3, off=2, n=4) == 0
        ends, dist = find_edit(P, text, 3, off=2, n=4)
        assert len(ends) == 0 and len(dist) == 0
        assert search_edit(P, text, 0, off=9, n=0) == 0
    # a pattern byte the text does not hold
    rng = np.random.default_rng(1200)
    T = np.asarray((65, 67, 71, 84), dtype=np.uint8)[rng.integers(0, 4, 20000)]
    P = T[9000:9024].copy()
    P[7] = ord("N")
    with uploaded(T) as text:
        assert check_bytes(text, T, P, 0) == 0
        assert check_bytes(text, T, P, 1) >= 1
        assert check_bytes(text, T, P, 3) >= 1


# ---- cap -------------------------------------------------------------------------------------------------------------------

def test_cap_count_and_missing_buffers():
    rng = np.random.default_rng(1300)
    T = np.asarray((65, 67, 71, 84), dtype=np.uint8)[rng.integers(0, 4, 50000)]
    P = T[777:787].copy()
    k = 2
    wends, wdist = edit_occurrences(10, byte_accepts(P), T, k)
    total = len(wends)
    assert total >= 50
    L = engine.lib()
    with uploaded(T) as text:
        ends = np.full(total, 7, dtype=np.uint64)
        dist = np.full(total, 9, dtype=np.uint8)
        c = ctypes.c_uint64(0)
        # one short: the true count, SMARTGPU_ERR_NOMEM
        assert L.smartgpu_find_edit64(P.ctypes.data, 10, k, text._h, 0, len(T), ends.ctypes.data, dist.ctypes.data, total - 1, ctypes.byref(c)) == ERR_NOMEM
        assert c.value == total and "room for %d" % (total - 1) in L.smartgpu_last_error().decode()
        with pytest.raises(SmartGpuError, match="%d occurrences" % total):
            find_edit(P, text, k, cap=total - 1)
        # cap = 0 with NULL buffers is a count
        c = ctypes.c_uint64(0)
        assert L.smartgpu_find_edit64(P.ctypes.data, 10, k, text._h, 0, len(T), None, None, 0, ctypes.byref(c)) == ERR_NOMEM and c.value == total
        c = ctypes.c_uint64(5)
        assert L.smartgpu_find_edit64(P.ctypes.data, 10, 0, text._h, 40000, 5, None, None, 0, ctypes.byref(c)) == 0 and c.value == 0
        # distances == NULL
        c = ctypes.c_uint64(0)
        assert L.smartgpu_find_edit64(P.ctypes.data, 10, k, text._h, 0, len(T), ends.ctypes.data, None, total, ctypes.byref(c)) == 0
        assert c.value == total and np.array_equal(ends, wends)
        # the classes form takes the same paths
        rows = byte_classes(P)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_find_edit_classes64(rows.ctypes.data, 10, k, text._h, 0, len(T), ends.ctypes.data, dist.ctypes.data, total - 1, ctypes.byref(c)) == ERR_NOMEM
        assert c.value == total
        # a range outside a real text is refused, nothing written
        c = ctypes.c_uint64(77)
        assert L.smartgpu_search_edit64(P.ctypes.data, 10, k, text._h, 1, len(T), ctypes.byref(c), None, None) == -3 and c.value == 77
        assert "outside the text" in L.smartgpu_last_error().decode()
        # the times of a count
        pre, run = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        assert L.smartgpu_search_edit64(P.ctypes.data, 10, k, text._h, 0, len(T), ctypes.byref(c), ctypes.byref(pre), ctypes.byref(run)) == 0
        assert c.value == total and pre.value >= 0.0 and run.value > 0.0


# ---- identities ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vals", [(65, 67, 71, 84), (0, 255)])
def test_the_packed_kernels_give_the_same_ends_and_distances(vals):
    """planes_edit_find is an independent kernel: the same bytes packed, the same pattern and k."""
    rng = np.random.default_rng(1400 + len(vals))
    n = 2 * WG_RUN + 4321
    T = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]
    with uploaded(T) as text:
        pt = PackedText.pack(text)
        try:
            for m, k in ((12, 1), (20, 3), (33, 7), (64, 7)):
                P = T[5000:5000 + m].copy()
                pends, pdist, pcount = pfind_edit(P, pt, k, cap=n)
                ends, dist = find_edit(P, text, k, cap=n)
                assert pcount == len(ends) > 0 and np.array_equal(ends, pends) and np.array_equal(dist, pdist), (vals, m, k)
                for off, ln in ((129, 40000), (8191, n - 8191)):
                    pends, pdist, pcount = pfind_edit(P, pt, k, off=off, n=ln, cap=n)
                    ends, dist = find_edit(P, text, k, off=off, n=ln, cap=n)
                    assert np.array_equal(ends, pends) and np.array_equal(dist, pdist), (vals, m, k, off)
        finally:
            pt.free()


def test_k_0_is_find_and_singleton_classes_are_the_byte_pattern():
    E = english()[:100003]
    with uploaded(E) as text:
        for P in (b"the", b" and the ", E[5000:5033].tobytes(), E[70000:70064].tobytes()):
            P = np.frombuffer(P, dtype=np.uint8)
            pos, count = find(P, text)
            ends, dist = find_edit(P, text, 0)
            assert count == len(ends) > 0 and np.array_equal(ends, pos + np.uint64(len(P) - 1)) and not dist.any()
            assert search_edit(P, text, 0) == count
            for k in (1, 3):
                ends, dist = find_edit(P, text, k, cap=len(E))
                cends, cdist = find_edit_classes(byte_classes(P), text, k, cap=len(E))
                assert np.array_equal(ends, cends) and np.array_equal(dist, cdist)
                assert search_edit_classes(byte_classes(P), text, k) == len(ends)


def test_classes_ignore_case_and_rows_by_hand():
    E = english()[:120001]
    fold = np.arange(256, dtype=np.uint8)
    fold[65:91] += 32
    with uploaded(E) as text:
        for word, k in ((b"aBRAHAM", 1), (b"THE LORD", 0), (b"the lord god", 2), (b"AnD iT cAmE tO pAsS, wHeN", 3)):
            P = np.frombuffer(word, dtype=np.uint8)
            rows = byte_classes(P, ignore_case=True)
            folded = lambda i, R, P=P: fold[R] == fold[P[i]]  # noqa: E731
            row = edit_row(len(P), folded, E)
            got = check(text, row, k, count=lambda t, k, off, n: search_edit_classes(rows, t, k, off=off, n=n),
                        find=lambda t, k, off, n, cap: find_edit_classes(rows, t, k, off=off, n=n, cap=cap), what=word)
            assert got >= 1, word
        # rows by hand: vowels, an EMPTY row (accepts nothing: one edit at least), a FULL row, digits and blanks
        rows = np.zeros((6, 32), dtype=np.uint8)
        for j, members in enumerate((b"tT", b"aeiou", b"", None, b" ,.;:", b"aeiouAEIOU")):
            for v in (range(256) if members is None else members):
                rows[j, v >> 3] |= 1 << (v & 7)
        assert not rows[2].any() and (rows[3] == 255).all()
        row = edit_row(6, class_accepts(rows), E)
        assert row.min() == 1
        for k in (0, 1, 2):
            got = check(text, row, k, count=lambda t, k, off, n: search_edit_classes(rows, t, k, off=off, n=n),
                        find=lambda t, k, off, n, cap: find_edit_classes(rows, t, k, off=off, n=n, cap=cap), what="by hand")
            assert (got == 0) == (k == 0)


# ---- the coalescing queue --------------------------------------------------------------------------------------------------

def test_a_call_behind_queued_horspool_launches():
    """Plan.launch calls wait in the coalescing queue; an edit call on the same text sends them first (device_ctx_flushed) and
    never enters the queue itself.  Both give their right answers."""
    from test_coalesce_gpu import cut
    rng = np.random.default_rng(1500)
    n = 3 * WG_RUN + 99
    T = rng.integers(0, 128, n).astype(np.uint8)
    pats = [cut(T, 1000 + 9000 * j, 16) for j in range(4)]
    for j, P in enumerate(pats):
        T[50000 + 100 * j:50000 + 100 * j + 16] = P
    raw = T.tobytes()

    def occurrences(P):
        c, at = 0, raw.find(P.tobytes())
        while at >= 0:
            c, at = c + 1, raw.find(P.tobytes(), at + 1)
        return c
    Q = T[20000:20020].copy()
    row = edit_row(20, byte_accepts(Q), T)
    default = engine.coalesce(8)
    try:
        with uploaded(T) as text:
            plans = [Plan("hor", P) for P in pats]
            try:
                engine.device_sync(0)
                l0, p0 = engine.coalesce_stats(0)
                for pl in plans:
                    pl.launch(text)
                got = check_bytes(text, T, Q, 2, row=row)  # the queue is sent here
                engine.device_sync(0)
                l1, p1 = engine.coalesce_stats(0)
                assert got >= 1
                assert [pl.result(0)[0] for pl in plans] == [occurrences(P) for P in pats]
                assert (l1 - l0, p1 - p0) == (len(plans), 1)  # the four launches were queued, and left as ONE pass
            finally:
                for pl in plans:
                    pl.free()
    finally:
        engine.device_sync(0)
        engine.coalesce(default)
