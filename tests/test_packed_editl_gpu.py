"""Edit distance for long patterns on packed texts on the GPU (planes_editl_scan, planes_editl_find): counts, end positions and
distances against the DEFINITION — Sellers' DP on the range, the oracle of tests/test_packed_edit.py — and, in every
comparison, the answers with SMARTGPU_PEDITL_ALL_BLOCKS against those with the cut-off.  Every comparison is exact equality;
no text is longer than 2^20 + 3 symbols."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (PackedText, pfind_edit, pfind_editl, pfind_sets_editl, psearch_edit, psearch_editl, psearch_sets_editl)  # noqa: E402

from test_packed_edit import byte_accepts, edit_occurrences, edit_row, set_accepts  # noqa: E402
from test_packed_edit_gpu import edited, other, random_text  # noqa: E402
from test_packed_editl import PIECE, RUN, WAVE_RUN, WG_RUN  # noqa: E402
from test_packed_text_gpu import VALUE_SETS  # noqa: E402

ACGT = (65, 67, 71, 84)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def check_row(D, pat, pt, k, off=0, n=None, what=None, sets=False):
    """Count, ends and distances of both calls, with the cut-off and with all blocks, against the oracle's row D (edit_row
    over the same range); returns a dict end -> distance."""
    at = np.flatnonzero(D <= k)
    wpos, wdist = (at + off).astype(np.uint64), D[at].astype(np.uint8)
    count, find = (psearch_sets_editl, pfind_sets_editl) if sets else (psearch_editl, pfind_editl)
    for all_blocks in (False, True):
        got = count(pat, pt, k, off=off, n=n, all_blocks=all_blocks)[0]
        assert got == len(wpos), (what, k, all_blocks, got, len(wpos))
        pos, dist, cnt = find(pat, pt, k, off=off, n=n, cap=max(len(wpos), 1), all_blocks=all_blocks)
        assert cnt == len(wpos) and pos is not None and pos.dtype == np.uint64 and dist.dtype == np.uint8, (what, k, all_blocks, cnt, len(wpos))
        assert np.array_equal(pos, wpos), (what, k, all_blocks)
        assert np.array_equal(dist, wdist), (what, k, all_blocks)
    return dict(zip(wpos.tolist(), wdist.tolist()))


def cut_patterns(T, vals, m):
    """The pattern cut from the text (repeated where the text is shorter) and the same with one symbol changed."""
    mid = max(len(T) - m, 0) // 2
    pats = [np.resize(T[mid:mid + m], m)]
    if len(vals) > 1:
        P = pats[0].copy()
        P[m // 2] = other(vals, P[m // 2])
        pats.append(P)
    return pats


# ---- 1. the old lengths: a second kernel for what the edit calls answer ---------------------------------------------------

@pytest.mark.parametrize("m", [1, 32, 33, 64])
@pytest.mark.parametrize("vals", VALUE_SETS)
def test_the_old_lengths_equal_the_edit_calls(vals, m):
    for n in (33, 4097):
        T = random_text(vals, n, 2100 + n)
        with PackedText.upload(T) as pt:
            for P in cut_patterns(T, vals, m):
                D = edit_row(m, byte_accepts(P), T)
                for k in (0, 3, 7):
                    found = check_row(D, P, pt, k, what=(vals, n, m))
                    pos, dist, cnt = pfind_edit(P, pt, k, cap=n)
                    assert cnt == len(found) == psearch_edit(P, pt, k)[0], (vals, n, m, k)
                    assert dict(zip(pos.tolist(), dist.tolist())) == found and list(found) == pos.tolist(), (vals, n, m, k)


# ---- 2. lengths and values ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [65, 96, 97, 128, 129, 255, 256])
@pytest.mark.parametrize("vals", VALUE_SETS)
def test_lengths_and_values(vals, m):
    for n in (1, 33, 4097):
        T = random_text(vals, n, 2200 + n)
        with PackedText.upload(T) as pt:
            for P in cut_patterns(T, vals, m):
                D = edit_row(m, byte_accepts(P), T)
                for k in (0, 7, 15, 31):
                    found = check_row(D, P, pt, k, what=(vals, n, m))
                    if n + k < m:
                        assert not found
            if m <= n:
                assert psearch_editl(cut_patterns(T, vals, m)[0], pt, 0)[0] >= 1  # the cut window itself


@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_the_longest_pattern_on_a_long_text(vals):
    n, m = 2**20 + 3, 256
    T = random_text(vals, n, 2300 + len(vals))
    P = cut_patterns(T, vals, m)[1]
    T[1000:1000 + m - 9] = np.delete(P, np.arange(20, 29))  # and a copy with nine symbols dropped
    D = edit_row(m, byte_accepts(P), T)
    with PackedText.upload(T) as pt:
        for k in (0, 7, 15, 31):
            found = check_row(D, P, pt, k, what=(vals, k))
            assert (1 in found.values()) == (k >= 1) and (found.get(1000 + m - 10) == 9) == (k >= 9)


# ---- 3. one planted edit at every block seam ---------------------------------------------------------------------------------

def seam_positions(m):
    js = {0, 1, m - 1}
    for b in range(32, m, 32):
        js |= {b - 1, b, b + 1}
    return sorted(j for j in js if 0 <= j < m)


@pytest.mark.parametrize("m", [97, 256])
@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_one_planted_edit_at_every_block_seam(vals, m):
    """At pattern positions 0, 1, m - 1 and around every multiple of 32 one substitution, one deletion and one insertion: the
    planted end is found at distance 1 with k = 1 and is absent with k = 0.  The guards are those of
    test_one_planted_edit_at_every_pattern_position: the symbol before a planted window differs from P[0], an inserted symbol
    from P[j - 1], and no insertion is planted before P[0]."""
    n = 4097
    P = random_text(vals, m, 300 + m + len(vals))
    at = (500, 1800, 3100)
    assert {0, 1, 31, 32, 33, 63, 64, 65, 95, 96, m - 1} <= set(seam_positions(m))
    for j in seam_positions(m):
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


# ---- 4. the budget's boundary --------------------------------------------------------------------------------------------------

def boundary_inputs():
    """(T, P, ends, planted distances): copies of a 256-symbol pattern with d = 0 .. 36 mixed edits."""
    m, n = 256, 16001
    rng = np.random.default_rng(5250)  # (chosen so that the assertion on the inputs in test_budget_boundary holds)
    T = random_text(ACGT, n, 6256)
    P = random_text(ACGT, m, 7256)
    ends = []
    for d in range(37):
        W = edited(P, d, rng, ACGT)
        a = 100 + d * 420
        T[a:a + len(W)] = W
        ends.append(a + len(W) - 1)
    D = edit_row(m, byte_accepts(P), T)
    return T, P, ends, D


def test_budget_boundary():
    T, P, ends, D = boundary_inputs()
    planted = [int(D[e]) for e in ends]
    # the inputs, by the oracle alone: a copy at exactly 31 and one above 31
    assert planted[0] == 0 and all(x <= d for d, x in enumerate(planted)) and max(planted) > 31 and all(x in planted for x in (7, 8, 15, 16, 30, 31))
    with PackedText.upload(T) as pt:
        for k in (0, 7, 8, 15, 16, 30, 31):
            found = check_row(D, P, pt, k, what=k)
            for e, x in zip(ends, planted):
                assert found.get(e) == (x if x <= k else None), (k, e, x)


# ---- 5. blocks switching on and off ----------------------------------------------------------------------------------------------

def plant_prefixes(T, P, at, lengths):
    """Prefixes of P, each followed by a symbol P does not continue with; returns the position behind the last one."""
    for length in lengths:
        if not 0 < length < len(P):
            continue
        T[at:at + length] = P[:length]
        T[at + length] = other(ACGT, P[length])
        at += length + 150
    return at


@pytest.mark.parametrize("m", [97, 256])
def test_planted_prefixes(m):
    n = 4097
    T = random_text(ACGT, n, 3100 + m)
    P = random_text(ACGT, m, 3200 + m)
    assert plant_prefixes(T, P, 300, (31, 32, 33, 64, 100, 200, m - 1)) < n
    D = edit_row(m, byte_accepts(P), T)
    with PackedText.upload(T) as pt:
        for k in (0, 7, 31):
            check_row(D, P, pt, k, what=(m, k))
    assert D.min() > 0  # (the inputs: prefixes only, no occurrence at k = 0)


def test_a_periodic_pattern_on_a_periodic_text():
    n, m = 20011, 256
    T = np.resize(np.asarray(ACGT[:3], dtype=np.uint8), n)
    T[5000] = ACGT[3]            # one foreign symbol, and one symbol dropped further on (the phase shifts)
    T = np.delete(T, 12000)
    P = np.resize(np.asarray(ACGT[:3], dtype=np.uint8), m)
    D = edit_row(m, byte_accepts(P), T)
    with PackedText.upload(T) as pt:
        for k in (0, 1, 31):
            found = check_row(D, P, pt, k, what=k)
            assert len(found) > (n - m) // 3 - 200
    assert 0 in D and 1 in D and 2 in D


def test_a_one_value_text_gives_every_distance():
    n, m, k = WAVE_RUN + 2 * RUN + 5, 256, 31
    T = np.full(n, 7, dtype=np.uint8)
    P = np.full(m, 7, dtype=np.uint8)
    D = edit_row(m, byte_accepts(P), T)
    with PackedText.upload(T) as pt:
        found = check_row(D, P, pt, k, what="one value")
    assert sorted(found) == list(range(m - 1 - k, n)) and set(found.values()) == set(range(32))


def test_prefixes_in_one_lanes_run_only():
    """Prefixes of the pattern, and a copy with five edits, planted in the run of ONE lane of a wave: that lane needs blocks its
    63 neighbours do not."""
    n, m = 2 * WAVE_RUN + 3, 256
    T = random_text(ACGT, n, 3300)
    P = random_text(ACGT, m, 3400)
    lane = 17 * RUN
    plant_prefixes(T, P, lane + 40, (200,))
    plant_prefixes(T, P, WAVE_RUN + 41 * RUN + 3, (100, 64))
    W = edited(P, 5, np.random.default_rng(3500), ACGT)
    T[lane + RUN - 30:lane + RUN - 30 + len(W)] = W   # it ends in the next lane's run
    D = edit_row(m, byte_accepts(P), T)
    e = lane + RUN - 30 + len(W) - 1
    assert 0 < D[e] <= 5 and np.count_nonzero(D <= 7) < 10  # (the inputs)
    with PackedText.upload(T) as pt:
        for k in (0, 4, 7, 31):
            found = check_row(D, P, pt, k, what=k)
            assert (e in found) == (D[e] <= k)


# ---- 6. seams of lanes, pieces, waves and workgroups -----------------------------------------------------------------------------

def test_seams_of_lanes_pieces_waves_and_workgroups():
    """A lane owns RUN consecutive end positions and loads them in pieces of PIECE, a wave 64 runs, a workgroup 256.
    Occurrences that END at the first and at the last owned position of each — exact copies, a copy with k = 31 insertions
    (it spans 287 symbols: the lane needs its whole warm-up) and a copy with 31 deletions."""
    m, k = 256, 31
    n = 6 * WG_RUN + 5
    T = random_text(ACGT, n, 800 + m)
    P = random_text(ACGT, m, 900 + m)
    ins = P.copy()
    for t in range(k):  # k symbols added, spread over the pattern, each different from the one before it
        j = 1 + (len(ins) - 2) * (t + 1) // (k + 1)
        ins = np.insert(ins, j, other(ACGT, ins[j - 1]))
    dele = np.delete(P, [1 + (m - 2) * (t + 1) // (k + 1) for t in range(k)])
    assert len(ins) == m + k and len(dele) == m - k
    first = {"lane": (5 * RUN, 20 * RUN, 40 * RUN), "piece": (7 * RUN + PIECE, 9 * RUN + 2 * PIECE, 11 * RUN + 3 * PIECE),
             "wave": (3 * WAVE_RUN, 2 * WAVE_RUN, 6 * WAVE_RUN), "workgroup": (WG_RUN, 2 * WG_RUN, 3 * WG_RUN)}
    last = {"lane": (14 * RUN - 1, 30 * RUN - 1, 50 * RUN - 1), "piece": (16 * RUN + PIECE - 1, 18 * RUN + 2 * PIECE - 1, 22 * RUN + 3 * PIECE - 1),
            "wave": (WAVE_RUN - 1, 5 * WAVE_RUN - 1, 7 * WAVE_RUN - 1), "workgroup": (4 * WG_RUN - 1, 5 * WG_RUN - 1, 6 * WG_RUN - 1)}
    planted = {}
    for where, ends in (("first", first), ("last", last)):
        for name, es in ends.items():
            for j, (e, W) in enumerate(zip(es, (P, ins, dele))):
                unit = PIECE if name == "piece" else RUN
                assert e < n and e not in planted and (e % unit == 0 if where == "first" else e % unit == unit - 1)
                assert all(abs(e - x) > 2 * (m + k) for x in planted)  # no planted window touches another
                T[e - len(W) + 1:e + 1] = W
                planted[e] = (where, name, j)
    assert len(planted) == 24
    D = edit_row(m, byte_accepts(P), T)
    with PackedText.upload(T) as pt:
        found = check_row(D, P, pt, k, what=(m, k))
        exact = check_row(D, P, pt, 0, what=(m, 0))
    for e, (where, name, j) in planted.items():
        assert found.get(e) == int(D[e]) <= k, (where, name, j, e)
        if j == 0:
            assert exact.get(e) == 0, (where, name, e)
    assert any(int(D[e]) == k for e in planted)  # (the inputs: an edited copy does need the whole budget)


# ---- 7. ranges -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k,short", [(100, 7, 93), (256, 31, 230)])
def test_ranges(m, k, short):
    """off and off + n that are no multiples of 32 or of the run; a pattern copy straddling off comes out at the substring's
    distance (> 0), one straddling off + n is not reported beyond the range; m > n is answered by deletions; n + k < m is 0 with
    no launch."""
    n_text = 3 * WAVE_RUN + 77
    T = random_text(ACGT, n_text, 1000 + m)
    P = random_text(ACGT, m, 1100 + m)
    half = m // 2
    for off, end in ((137, 1000 + 3), (RUN + 1, WAVE_RUN + 2 * RUN - 1), (WAVE_RUN - 3, 2 * WAVE_RUN + 45), (269, n_text), (133, 431)):
        assert off % 32 and end % 32 and off % RUN and end % RUN and off >= m - half
        T2 = T.copy()
        T2[off - (m - half):off + half] = P          # a copy straddling off: its last `half` symbols are in the range
        if end < n_text:
            T2[end - half:end + (m - half)] = P      # and one straddling off + n
        D = edit_row(m, byte_accepts(P), T2, off, end - off)
        e = off + half - 1
        assert edit_row(m, byte_accepts(P), T2[:off + half])[e] == 0 and D[e - off] >= m - half  # (the inputs: exact in the text, not in the range)
        with PackedText.upload(T2) as pt:
            for kk in (0, k):
                found = check_row(D, P, pt, kk, off=off, n=end - off, what=(m, kk, off, end))
                assert all(off <= x < end for x in found)
                assert found.get(e) == (int(D[e - off]) if D[e - off] <= kk else None), (m, kk, off)
    # m > n with n + k >= m: a range that holds the pattern less m - short symbols and nothing else
    cut = 5000
    T[cut:cut + short] = np.delete(P, np.arange(1, m - short + 1))
    D = edit_row(m, byte_accepts(P), T, cut, short)
    with PackedText.upload(T) as pt:
        found = check_row(D, P, pt, k, off=cut, n=short, what=(m, k, "m > n"))
        assert short < m and found.get(cut + short - 1) == m - short <= k, (m, k, found)
        # n + k < m: count 0, no launch
        for all_blocks in (False, True):
            cnt, pre, run = psearch_editl(P, pt, k, off=cut, n=m - k - 1, all_blocks=all_blocks)
            assert cnt == 0 and run == 0.0
            pos, dist, cnt = pfind_editl(P, pt, k, off=cut, n=m - k - 1, all_blocks=all_blocks)
            assert cnt == 0 and len(pos) == 0 and len(dist) == 0
        assert psearch_editl(P, pt, k, off=cut, n=0)[0] == 0
        with pytest.raises(smart_amd.SmartGpuError) as err:
            pfind_editl(P, pt, k, off=n_text - 10, n=11)  # a range outside the text
        assert "rc=-3" in str(err.value) and "outside the packed text" in str(err.value)
        with pytest.raises(smart_amd.SmartGpuError):
            psearch_editl(P, pt, k, off=n_text + 1, n=0)


# ---- 8. sets ---------------------------------------------------------------------------------------------------------------------

def test_singleton_sets_equal_the_byte_pattern_calls():
    n = 2**16 + 5
    for vals in (ACGT, (65, 67, 84), (0, 255)):
        T = random_text(vals, n, 1300 + len(vals))
        with PackedText.upload(T) as pt:
            for m, k in ((33, 3), (100, 7), (256, 31)):
                P = T[777:777 + m].copy()
                P[m // 2] = other(vals, P[m // 2])
                sets = np.array([1 << sorted(vals).index(b) for b in P.tolist()], dtype=np.uint8)
                for all_blocks in (False, True):
                    assert psearch_sets_editl(sets, pt, k, all_blocks=all_blocks)[0] == psearch_editl(P, pt, k)[0]
                    a, b = pfind_sets_editl(sets, pt, k, all_blocks=all_blocks), pfind_editl(P, pt, k)
                    assert a[2] == b[2] >= 1 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (vals, m, k)


MOTIF = "GGNCCWRTATAWAW" + "N" * 11 + "TATAWAWRRGGNCCWRTA" + "N" * 23 + "CCWRTATAWAWGGACGTR" + "N" * 7 + "WRTATAWAWGGNCCRTTAGCAWGGAC"


def test_iupac_motif_against_the_oracle():
    n = 2**16 + 5
    assert 115 <= len(MOTIF) <= 125
    T = random_text(ACGT, n, 1401)
    inst = np.frombuffer(MOTIF.replace("N", "C").replace("W", "A").replace("R", "G").encode(), dtype=np.uint8)
    T[3000:3000 + len(inst)] = inst
    T[40000:40000 + len(inst) - 1] = np.delete(inst, 5)   # one deletion
    T[50000:50000 + len(inst) + 1] = np.insert(inst, 3, other(ACGT, inst[2]))  # one insertion
    with PackedText.upload(T) as pt:
        sets = pt.iupac(MOTIF)
        D = edit_row(len(sets), set_accepts(sets, ACGT), T)
        for k in (0, 1, 9, 31):
            found = check_row(D, sets, pt, k, what=k, sets=True)
            assert found.get(3000 + len(inst) - 1) == 0
            if k >= 1:
                assert found.get(40000 + len(inst) - 2) <= 1 and found.get(50000 + len(inst)) <= 1


def test_an_empty_set_behaves_as_a_foreign_byte():
    n = 4097
    T = random_text(ACGT, n, 1500)
    with PackedText.upload(T) as pt:
        for m, k in ((70, 2), (256, 9)):
            P = T[1000:1000 + m].copy()
            P[m // 3] = ord("N")
            P[m - 2] = ord("N")
            sets = np.array([0 if b == ord("N") else 1 << ACGT.index(b) for b in P.tolist()], dtype=np.uint8)
            D = edit_row(m, byte_accepts(P), T)
            assert np.array_equal(D, edit_row(m, set_accepts(sets, ACGT), T))
            found = check_row(D, P, pt, k, what=(m, k, "foreign"))
            assert found == check_row(D, sets, pt, k, what=(m, k, "empty"), sets=True)
            assert found.get(1000 + m - 1) == 2 and not check_row(D, P, pt, 1, what=(m, 1))
            full = np.full(m, 15, dtype=np.uint8)  # full sets: every end position from m - 1 on at distance 0
            Df = edit_row(m, set_accepts(full, ACGT), T)
            ff = check_row(Df, full, pt, 0, what=(m, "full"), sets=True)
            assert sorted(ff) == list(range(m - 1, n))


def test_a_set_that_names_a_code_the_text_does_not_hold_is_refused():
    T = random_text((65, 67, 84), 1000, 1600)
    with PackedText.upload(T) as pt:
        sets = np.array([1, 2, 4, 1] * 40 + [8, 1], dtype=np.uint8)
        for call in (lambda: psearch_sets_editl(sets, pt, 1), lambda: pfind_sets_editl(sets, pt, 1)):
            with pytest.raises(smart_amd.SmartGpuError) as e:
                call()
            assert "rc=-3" in str(e.value) and "position 160" in str(e.value)


# ---- 9. cap ----------------------------------------------------------------------------------------------------------------------

def test_cap_and_count():
    L = smart_amd.lib()
    m, k = 100, 31
    T = random_text((0, 255), 5000, 7000)
    P = T[10:10 + m].copy()
    with PackedText.upload(T) as pt:
        wpos, wdist = edit_occurrences(m, byte_accepts(P), T, k)
        assert len(wpos) > 10
        for flags in (0, 1):
            # cap smaller than the count: SMARTGPU_ERR_NOMEM with count filled; cap = 0 with no buffer is a count
            out = np.zeros(4, dtype=np.uint64)
            dist = np.zeros(4, dtype=np.uint8)
            c = ctypes.c_uint64(0)
            assert L.smartgpu_pfind_editl64(P.ctypes.data, m, k, flags, pt._h, 0, len(T), out.ctypes.data, dist.ctypes.data, 4, ctypes.byref(c)) == -5
            assert c.value == len(wpos)
            c = ctypes.c_uint64(0)
            assert L.smartgpu_pfind_editl64(P.ctypes.data, m, k, flags, pt._h, 0, len(T), None, None, 0, ctypes.byref(c)) == -5
            assert c.value == len(wpos) == psearch_editl(P, pt, k, all_blocks=bool(flags))[0]
            # distances NULL with ends given
            out = np.zeros(len(wpos), dtype=np.uint64)
            c = ctypes.c_uint64(0)
            assert L.smartgpu_pfind_editl64(P.ctypes.data, m, k, flags, pt._h, 0, len(T), out.ctypes.data, None, len(out), ctypes.byref(c)) == 0
            assert c.value == len(wpos) and np.array_equal(out, wpos)
        assert pfind_editl(P, pt, k, cap=4) == (None, None, len(wpos))
        assert pfind_editl(P, pt, k, cap=0) == (None, None, len(wpos))
        # nothing within the budget: a count of 0 needs no room
        never = np.full(200, ord("N"), dtype=np.uint8)
        c = ctypes.c_uint64(9)
        assert L.smartgpu_pfind_editl64(never.ctypes.data, 200, 31, 0, pt._h, 0, len(T), None, None, 0, ctypes.byref(c)) == 0 and c.value == 0
        with pytest.raises(smart_amd.SmartGpuError):
            psearch_editl(P, pt, 32)
        with pytest.raises(smart_amd.SmartGpuError):
            psearch_editl(np.full(257, 0, dtype=np.uint8), pt, 1)
