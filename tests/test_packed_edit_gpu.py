"""Occurrences within edit distance k on packed texts on the GPU (planes_edit_scan, planes_edit_find): counts, end positions
and distances against the DEFINITION — Sellers' DP on the range, computed row by row with numpy (tests/test_packed_edit.py,
where it is checked against the plain DP).  Every comparison is exact equality; no text here is longer than 2^20 + 3 symbols — later trips of the grid-stride
loop and positions beyond 2^32 are in tests/test_packed_at_size_gpu.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (PackedText, pfind, pfind_edit, pfind_mis, pfind_sets_edit, psearch_edit, psearch_sets_edit)  # noqa: E402

from test_packed_edit import RUN, WAVE_RUN, WG_RUN, byte_accepts, edit_occurrences, edit_row, set_accepts  # noqa: E402
from test_packed_text_gpu import VALUE_SETS  # noqa: E402

ACGT = (65, 67, 71, 84)
MS = [1, 2, 8, 31, 32, 33, 63, 64]
KS = [0, 1, 3, 7]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def random_text(vals, n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]


def other(vals, v):
    return next(x for x in vals if x != v)


def check_row(D, pat, pt, k, off=0, n=None, what=None, sets=False):
    """Count, ends and distances of both calls against the oracle's row D (edit_row over the same range); returns a dict
    end -> distance."""
    at = np.flatnonzero(D <= k)
    wpos, wdist = (at + off).astype(np.uint64), D[at].astype(np.uint8)
    count, find = (psearch_sets_edit, pfind_sets_edit) if sets else (psearch_edit, pfind_edit)
    got = count(pat, pt, k, off=off, n=n)[0]
    assert got == len(wpos), (what, k, got, len(wpos))
    pos, dist, cnt = find(pat, pt, k, off=off, n=n, cap=max(len(wpos), 1))
    assert cnt == len(wpos) and pos is not None and pos.dtype == np.uint64 and dist.dtype == np.uint8, (what, k, cnt, len(wpos))
    assert np.array_equal(pos, wpos), (what, k)
    assert np.array_equal(dist, wdist), (what, k)
    return dict(zip(pos.tolist(), dist.tolist()))


def check(P, T, pt, k, off=0, n=None, what=None):
    P = np.asarray(P, dtype=np.uint8)
    return check_row(edit_row(len(P), byte_accepts(P), T, off, n), P, pt, k, off, n, what)


# ---- 1. values and lengths ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", [1, 33, 4097, 2**20 + 3])
@pytest.mark.parametrize("vals", VALUE_SETS)
def test_values_and_lengths(vals, n, m):
    """The pattern cut from the text (repeated where the text is shorter) and the same with one symbol changed; k = 0 is the
    exact matcher's positions plus m - 1."""
    T = random_text(vals, n, 2000 + n)
    mid = max(n - m, 0) // 2
    pats = [np.resize(T[mid:mid + m], m)]
    if len(vals) > 1:
        P = pats[0].copy()
        P[m // 2] = other(vals, P[m // 2])
        pats.append(P)
    with PackedText.upload(T) as pt:
        for P in pats:
            D = edit_row(m, byte_accepts(P), T)
            for k in KS:
                found = check_row(D, P, pt, k, what=(vals, n, m))
                if n + k < m:
                    assert not found
            if m <= n:
                wpos, wcnt = pfind(P, pt, cap=n)
                gpos, gdist, gcnt = pfind_edit(P, pt, 0, cap=n)
                assert gcnt == wcnt and np.array_equal(gpos, wpos + np.uint64(m - 1)) and not gdist.any(), (vals, n, m)
        if m <= n:
            assert psearch_edit(pats[0], pt, 0)[0] >= 1  # the cut window itself


# ---- 2. planted edits --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [40, 64])
@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_one_planted_edit_at_every_pattern_position(vals, m):
    """At each pattern position one substitution, one deletion (a text symbol removed) and one insertion (a text symbol
    added): the planted end is found at distance 1 with k = 1 and is absent with k = 0.  The symbol before a planted window
    differs from P[0] and an inserted symbol from P[j - 1], so that no planted window is an exact occurrence; an insertion
    before P[0] is no edit (the symbol is text before the match) and is not planted."""
    n = 4097
    P = random_text(vals, m, 300 + m + len(vals))
    at = (500, 1800, 3100)
    for j in range(m):
        T = random_text(vals, n, 400 + j)
        sub = P.copy()
        sub[j] = other(vals, sub[j])
        windows = [sub, np.delete(P, j)]
        if j > 0:
            windows.append(np.insert(P, j, other(vals, P[j - 1])))
        ends = []
        for a, W in zip(at, windows):
            T[a - 1] = other(vals, P[0])
            T[a:a + len(W)] = W
            ends.append(a + len(W) - 1)
        D = edit_row(m, byte_accepts(P), T)
        with PackedText.upload(T) as pt:
            found1 = check_row(D, P, pt, 1, what=(vals, m, j))
            found0 = check_row(D, P, pt, 0, what=(vals, m, j))
        for e in ends:
            assert found1.get(e) == 1 and e not in found0, (vals, m, j, e)


# ---- 3. the budget's boundary ------------------------------------------------------------------------------------------

def edited(P, d, rng, vals):
    """P with d edits at distinct positions >= 1, the three kinds in turn."""
    W = list(P.tolist())
    for t, j in enumerate(sorted(rng.choice(np.arange(1, len(P) - 1), size=d, replace=False).tolist(), reverse=True)):
        if t % 3 == 0:
            W[j] = other(vals, W[j])
        elif t % 3 == 1:
            del W[j]
        else:
            W.insert(j, other(vals, W[j - 1]))
    return np.asarray(W, dtype=np.uint8)


@pytest.mark.parametrize("m", [33, 64])
def test_budget_boundary(m):
    """Windows planted with d = 0 .. 9 edits that mix the three kinds: k = 7 reports those with D <= 7, at the oracle's
    distances, and every smaller k its own share."""
    n = 4097
    rng = np.random.default_rng(500 + m)
    T = random_text(ACGT, n, 600 + m)
    P = random_text(ACGT, m, 700 + m)
    ends = []
    for d in range(10):
        W = edited(P, d, rng, ACGT)
        a = 100 + d * 390
        T[a:a + len(W)] = W
        ends.append(a + len(W) - 1)
    D = edit_row(m, byte_accepts(P), T)
    planted = [int(D[e]) for e in ends]
    assert planted[0] == 0 and all(x <= d for d, x in enumerate(planted)) and max(planted) > 7 and 7 in planted  # (the inputs, by the oracle alone)
    with PackedText.upload(T) as pt:
        for k in range(8):
            found = check_row(D, P, pt, k, what=(m, k))
            for e, x in zip(ends, planted):
                assert found.get(e) == (x if x <= k else None), (m, k, e, x)


# ---- 4. lane, wave and workgroup seams -----------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(64, 7), (33, 3), (20, 1)])
def test_seams_of_lanes_waves_and_workgroups(m, k):
    """A lane owns RUN consecutive end positions, a wave 64 such runs, a workgroup 256.  Occurrences that END at the first and
    at the last owned position of a lane, of a wave and of a workgroup — exact copies, a copy with k insertions (it spans
    m + k symbols: the lane needs its whole warm-up) and a copy with k deletions."""
    n = 6 * WG_RUN + 5
    T = random_text(ACGT, n, 800 + m)
    P = random_text(ACGT, m, 900 + m)
    ins = P.copy()
    for t in range(k):  # k symbols added, spread over the pattern, each different from the one before it
        j = 1 + (len(ins) - 2) * (t + 1) // (k + 1)
        ins = np.insert(ins, j, other(ACGT, ins[j - 1]))
    dele = np.delete(P, [1 + (m - 2) * (t + 1) // (k + 1) for t in range(k)])
    assert len(ins) == m + k and len(dele) == m - k
    first = {"lane": (5 * RUN, 20 * RUN, 40 * RUN), "wave": (3 * WAVE_RUN, 2 * WAVE_RUN, 6 * WAVE_RUN), "workgroup": (WG_RUN, 2 * WG_RUN, 3 * WG_RUN)}
    last = {"lane": (9 * RUN - 1, 30 * RUN - 1, 50 * RUN - 1), "wave": (WAVE_RUN - 1, 5 * WAVE_RUN - 1, 7 * WAVE_RUN - 1), "workgroup": (4 * WG_RUN - 1, 5 * WG_RUN - 1, 6 * WG_RUN - 1)}
    planted = {}
    for where, ends in (("first", first), ("last", last)):
        for name, es in ends.items():
            for j, (e, W) in enumerate(zip(es, (P, ins, dele))):
                if e is None:
                    continue
                assert e < n and e not in planted and (e % RUN == 0 if where == "first" else e % RUN == RUN - 1)
                T[e - len(W) + 1:e + 1] = W
                planted[e] = (where, name, j)
    assert len(planted) == 18
    D = edit_row(m, byte_accepts(P), T)
    with PackedText.upload(T) as pt:
        found = check_row(D, P, pt, k, what=(m, k))
        exact = check_row(D, P, pt, 0, what=(m, 0))
    for e, (where, name, j) in planted.items():
        assert found.get(e) == int(D[e]) <= k, (m, k, where, name, j, e)
        if j == 0:
            assert exact.get(e) == 0, (m, where, name, e)
    assert any(int(D[e]) == k for e in planted)  # (the inputs: an edited copy does need the whole budget)


# ---- 5. ranges -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(8, 1), (40, 3), (64, 7)])
def test_ranges(m, k):
    """off and off + n that are no multiples of 32 or 128; a pattern copy straddling off comes out at the substring's distance
    (> 0), one straddling off + n is not reported beyond the range; m > n is answered by deletions; n + k < m is 0."""
    n_text = 3 * WAVE_RUN + 77
    T = random_text(ACGT, n_text, 1000 + m)
    P = random_text(ACGT, m, 1100 + m)
    half = m // 2
    for off, end in ((37, 1000 + 3), (RUN + 1, WAVE_RUN + 2 * RUN - 1), (WAVE_RUN - 3, 2 * WAVE_RUN + 45), (69, n_text), (33, 131)):
        assert off % 32 and end % 32 and off >= m - half
        T2 = T.copy()
        T2[off - (m - half):off + half] = P          # a copy straddling off: its last `half` symbols are in the range
        if end < n_text:
            T2[end - half:end + (m - half)] = P      # and one straddling off + n
        D = edit_row(m, byte_accepts(P), T2, off, end - off)
        e = off + half - 1
        assert edit_row(m, byte_accepts(P), T2)[e] == 0 and D[e - off] >= m - half  # (the inputs: exact in the text, not in the range)
        with PackedText.upload(T2) as pt:
            for kk in (0, k):
                found = check_row(D, P, pt, kk, off=off, n=end - off, what=(m, kk, off, end))
                assert all(off <= x < end for x in found)
                assert found.get(e) == (int(D[e - off]) if D[e - off] <= kk else None), (m, kk, off)
    # m > n with n + k >= m: a range that holds the pattern less k symbols and nothing else
    cut, short = 5000, m - k
    T[cut:cut + short] = np.delete(P, np.arange(1, k + 1))
    D = edit_row(m, byte_accepts(P), T, cut, short)
    with PackedText.upload(T) as pt:
        found = check_row(D, P, pt, k, off=cut, n=short, what=(m, k, "m > n"))
        assert short < m and found.get(cut + short - 1) == k, (m, k, found)
        # n + k < m: count 0
        assert psearch_edit(P, pt, k, off=cut, n=short - 1)[0] == 0
        pos, dist, cnt = pfind_edit(P, pt, k, off=cut, n=short - 1)
        assert cnt == 0 and len(pos) == 0 and len(dist) == 0
        assert psearch_edit(P, pt, k, off=cut, n=0)[0] == 0
        with pytest.raises(smart_amd.SmartGpuError):
            pfind_edit(P, pt, k, off=n_text - 10, n=11)  # a range outside the text


# ---- 6. k >= m -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 3, 7])
def test_k_at_least_m(m):
    n = 5003
    T = random_text(ACGT, n, 7200 + m)
    P = T[100:100 + m].copy()
    with PackedText.upload(T) as pt:
        found = check(P, T, pt, 7, what=m)
        assert sorted(found) == list(range(n)) and max(found.values()) <= m and found[100 + m - 1] == 0
        found = check(P, T, pt, 7, off=1000, n=301, what=(m, "range"))
        assert sorted(found) == list(range(1000, 1301))


# ---- 7. sets ---------------------------------------------------------------------------------------------------------------

def test_singleton_sets_equal_the_byte_pattern_calls():
    n = 2**16 + 5
    for vals in (ACGT, (65, 67, 84), (0, 255)):
        T = random_text(vals, n, 1300 + len(vals))
        with PackedText.upload(T) as pt:
            for m, k in ((8, 1), (33, 3), (64, 7)):
                P = T[777:777 + m].copy()
                P[m // 2] = other(vals, P[m // 2])
                sets = np.array([1 << sorted(vals).index(b) for b in P.tolist()], dtype=np.uint8)
                assert psearch_sets_edit(sets, pt, k)[0] == psearch_edit(P, pt, k)[0]
                a, b = pfind_sets_edit(sets, pt, k), pfind_edit(P, pt, k)
                assert a[2] == b[2] >= 1 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (vals, m, k)


@pytest.mark.parametrize("motif", ["GGNCCWRTATAWAW", "TATAWAWNNNNNNNNNNNNNNNNNNNNNRRGGNCCWRTATAWAW"])
def test_iupac_motif_against_the_oracle(motif):
    n = 2**16 + 5
    T = random_text(ACGT, n, 1401)
    inst = np.frombuffer(motif.replace("N", "C").replace("W", "A").replace("R", "G").encode(), dtype=np.uint8)
    T[3000:3000 + len(inst)] = inst
    T[40000:40000 + len(inst) - 1] = np.delete(inst, 5)   # one deletion
    T[50000:50000 + len(inst) + 1] = np.insert(inst, 3, other(ACGT, inst[2]))  # one insertion
    with PackedText.upload(T) as pt:
        sets = pt.iupac(motif)
        D = edit_row(len(sets), set_accepts(sets, ACGT), T)
        for k in (0, 1, 2):
            found = check_row(D, sets, pt, k, what=(motif, k), sets=True)
            assert found.get(3000 + len(inst) - 1) == 0
            if k >= 1:
                assert found.get(40000 + len(inst) - 2) <= 1 and found.get(50000 + len(inst)) <= 1


def test_an_empty_set_behaves_as_a_foreign_byte():
    n = 4097
    T = random_text(ACGT, n, 1500)
    with PackedText.upload(T) as pt:
        for m, k in ((8, 1), (40, 2)):
            P = T[1000:1000 + m].copy()
            P[m // 3] = ord("N")
            sets = np.array([0 if b == ord("N") else 1 << ACGT.index(b) for b in P.tolist()], dtype=np.uint8)
            D = edit_row(m, byte_accepts(P), T)
            assert np.array_equal(D, edit_row(m, set_accepts(sets, ACGT), T))
            found = check_row(D, P, pt, k, what=(m, k, "foreign"))
            assert found == check_row(D, sets, pt, k, what=(m, k, "empty"), sets=True)
            assert found.get(1000 + m - 1) == 1 and not check_row(D, P, pt, 0, what=(m, 0))
            full = np.full(m, 15, dtype=np.uint8)  # full sets: every end position from m - 1 on at distance 0
            Df = edit_row(m, set_accepts(full, ACGT), T)
            ff = check_row(Df, full, pt, 0, what=(m, "full"), sets=True)
            assert sorted(ff) == list(range(m - 1, n))


def test_a_set_that_names_a_code_the_text_does_not_hold_is_refused():
    T = random_text((65, 67, 84), 1000, 1600)
    with PackedText.upload(T) as pt:
        sets = np.array([1, 2, 4, 1, 8, 1], dtype=np.uint8)
        for call in (lambda: psearch_sets_edit(sets, pt, 1), lambda: pfind_sets_edit(sets, pt, 1)):
            with pytest.raises(smart_amd.SmartGpuError) as e:
                call()
            assert "rc=-3" in str(e.value) and "position 4" in str(e.value)


# ---- 8. relation to the Hamming calls --------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(8, 1), (20, 2), (40, 3), (64, 7)])
def test_every_hamming_occurrence_is_an_edit_occurrence(m, k):
    n = 2**16 + 5
    T = random_text(ACGT, n, 1700 + m)
    P = T[9000:9000 + m].copy()
    for j in range(0, m, max(m // (k + 1), 1)):
        T[20000 + j] = other(ACGT, T[20000 + j])
    T[30000:30000 + m] = P
    for j in list(range(0, m, max(m // (k + 1), 1)))[:k]:
        T[30000 + j] = other(ACGT, P[j])
    with PackedText.upload(T) as pt:
        spos, sdist, scnt = pfind_mis(P, pt, k)
        epos, edist, ecnt = pfind_edit(P, pt, k)
        assert scnt >= 2 and 30000 in spos.tolist()
        ends = dict(zip(epos.tolist(), edist.tolist()))
        for s, d in zip(spos.tolist(), sdist.tolist()):
            assert s + m - 1 in ends and ends[s + m - 1] <= d, (m, k, s, d)


# ---- 9. cap smaller than the count -----------------------------------------------------------------------------------------

def test_host_decisions():
    L = smart_amd.lib()
    T = random_text(ACGT, 5000, 7000)
    P = T[10:14].copy()
    with PackedText.upload(T) as pt:
        wpos, wdist = edit_occurrences(4, byte_accepts(P), T, 1)
        assert len(wpos) > 10
        # cap smaller than the count: SMARTGPU_ERR_NOMEM with count filled; cap = 0 with no buffer is a count
        out = np.zeros(4, dtype=np.uint64)
        dist = np.zeros(4, dtype=np.uint8)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_edit64(P.ctypes.data, 4, 1, pt._h, 0, len(T), out.ctypes.data, dist.ctypes.data, 4, ctypes.byref(c)) == -5
        assert c.value == len(wpos)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_edit64(P.ctypes.data, 4, 1, pt._h, 0, len(T), None, None, 0, ctypes.byref(c)) == -5
        assert c.value == len(wpos)
        # distances NULL with ends given
        out = np.zeros(len(wpos), dtype=np.uint64)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_edit64(P.ctypes.data, 4, 1, pt._h, 0, len(T), out.ctypes.data, None, len(out), ctypes.byref(c)) == 0
        assert c.value == len(wpos) and np.array_equal(out, wpos)
        assert pfind_edit(P, pt, 1, cap=4) == (None, None, len(wpos))
        assert pfind_edit(P, pt, 1, cap=0) == (None, None, len(wpos))
        # nothing within the budget: a count of 0 needs no room
        never = np.full(12, ord("N"), dtype=np.uint8)
        c = ctypes.c_uint64(9)
        assert L.smartgpu_pfind_edit64(never.ctypes.data, 12, 7, pt._h, 0, len(T), None, None, 0, ctypes.byref(c)) == 0 and c.value == 0
        with pytest.raises(smart_amd.SmartGpuError):
            psearch_edit(P, pt, 8)
        with pytest.raises(smart_amd.SmartGpuError):
            psearch_edit(np.full(65, 65, dtype=np.uint8), pt, 1)
