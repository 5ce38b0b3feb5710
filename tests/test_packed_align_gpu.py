"""Starts and alignments of edit-distance occurrences on the GPU (planes_edit_align): starts, distances and operations
against the DEFINITION — the plain DP of tests/test_packed_align.py (align_many, held there to the cell-by-cell align_one).
Every comparison is exact equality; no text here is longer than 2^20 + 3 symbols — ends beyond 2^32 are in
tests/test_packed_at_size_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import PackedText, edit_cigar, palign_edit, palign_sets_edit, pfind_edit, pfind_edit_align, pfind_sets_edit  # noqa: E402

from test_packed_align import DEL, EQ, INS, NONE_DIST, NONE_START, SUB, align_many, replay, unpack_ops  # noqa: E402
from test_packed_edit import byte_accepts, edit_row, set_accepts  # noqa: E402
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


def check(pat, accepts, T, pt, k, ends, off=0, n=None, what=None, sets=False):
    """Both forms of the call (with and without ops) against the oracle; returns (starts, distances, ops)."""
    call = palign_sets_edit if sets else palign_edit
    ends = np.asarray(ends, dtype=np.uint64)
    wstarts, wdist, wops = align_many(len(pat), accepts, T, ends, k, off)
    starts, dist, ops = call(pat, pt, k, ends, off=off, n=n)
    assert starts.dtype == np.uint64 and dist.dtype == np.uint8 and ops.dtype == np.uint64 and ops.shape == (len(ends), 3), what
    assert np.array_equal(starts, wstarts), (what, k)
    assert np.array_equal(dist, wdist), (what, k)
    assert np.array_equal(ops, wops), (what, k)
    s2, d2, o2 = call(pat, pt, k, ends, off=off, n=n, ops=False)
    assert o2 is None and np.array_equal(s2, wstarts) and np.array_equal(d2, wdist), (what, k, "ops=False")
    return starts, dist, ops


# ---- 1. lengths and values -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", [1, 33, 4097])
@pytest.mark.parametrize("vals", VALUE_SETS)
def test_lengths_and_values(vals, n, m):
    """The pattern cut from the text (repeated where the text is shorter) and the same with one symbol changed; the ends are
    the find's.  k = 0: every start is e - m + 1 and the operations are m times '='.  k >= m (m = 1, 2) holds the empty
    match s = e + 1 with m 'D's wherever no symbol of the pattern is near."""
    T = random_text(vals, n, 2000 + n)
    mid = max(n - m, 0) // 2
    pats = [np.resize(T[mid:mid + m], m)]
    if len(vals) > 1:
        P = pats[0].copy()
        P[m // 2] = other(vals, P[m // 2])
        pats.append(P)
    empty = 0
    with PackedText.upload(T) as pt:
        for P in pats:
            for k in KS:
                ends, fdist, cnt = pfind_edit(P, pt, k, cap=n)
                assert ends is not None and cnt == len(ends)
                starts, dist, ops = check(P, byte_accepts(P), T, pt, k, ends, what=(vals, n, m))
                assert np.array_equal(dist, fdist), (vals, n, m, k)  # the distances are the find's
                assert (starts <= ends + np.uint64(1)).all()
                if k == 0:
                    assert np.array_equal(starts, ends - np.uint64(m - 1)), (vals, n, m)
                    assert all(unpack_ops(r) == [EQ] * m for r in ops), (vals, n, m)
                hollow = starts == ends + np.uint64(1)
                assert all(unpack_ops(r) == [DEL] * m for r in ops[hollow])
                empty += int(hollow.sum())
    if m == 1 and len(vals) > 1 and n > 1:
        assert empty > 0  # (the inputs: the empty match was met — every end whose symbol is not the pattern's)


# ---- 2. clipping and dword edges -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(8, 1), (31, 3), (32, 7), (33, 0), (64, 7)])
@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_clipping_and_dword_edges(vals, m, k):
    """Ranges that start at off: the ends off .. off + m + k (every walk shorter than m + k columns, down to one), every e with
    e % 32 in {0, 31} below 96, and the last end of the text.  No start lies before off."""
    n = 4097
    T = random_text(vals, n, 2100 + m)
    P = T[2040:2040 + m].copy()
    for off in (0, 1, 31, 32, 33, 95, 97):
        # the whole pattern one symbol after off (a match whose walk is clipped), then one symbol BEFORE off (a match the range
        # cuts: inside the range it starts at off, at distance 1, whatever the symbol before off is)
        for at in (off + 1, off - 1):
            if at < 0:
                continue
            T2 = T.copy()
            T2[at:at + m] = P
            with PackedText.upload(T2) as pt:
                ends = set(range(off, off + m + k + 1)) | {e for e in range(96) if e % 32 in (0, 31) and e >= off} | {n - 1}
                ends = np.array(sorted(ends), dtype=np.uint64)
                starts, dist, _ = check(P, byte_accepts(P), T2, pt, k, ends, off=off, n=n - off, what=(vals, m, k, off, at))
            hit = dist != NONE_DIST
            assert (starts[hit] >= off).all() and (starts[~hit] == NONE_START).all()
            x = ends.tolist().index(at + m - 1)
            if at > off:
                assert (int(starts[x]), int(dist[x])) == (at, 0)
            elif k >= 1:
                assert int(dist[x]) <= 1 and int(starts[x]) >= off


# ---- 3. planted edits ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [40, 64])
@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_one_planted_edit_at_every_pattern_position(vals, m):
    """One substitution, one deletion and one insertion at every pattern position (the construction of
    tests/test_packed_edit_gpu.py), all positions in ONE text.  Compared against the oracle, not the planted offset — a
    substitution at position 0 legitimately yields the shorter match that starts one later — and every operation sequence
    replays: '=' on accepted symbols, 'X' on others, m pattern symbols, e - s + 1 text symbols, X + I + D = d."""
    P = random_text(vals, m, 300 + m + len(vals))
    gap = m + 16
    n = 3 * m * gap + 64
    T = random_text(vals, n, 400 + m)
    ends = []
    a = 8
    for j in range(m):
        sub = P.copy()
        sub[j] = other(vals, sub[j])
        windows = [sub, np.delete(P, j)]
        if j > 0:
            windows.append(np.insert(P, j, other(vals, P[j - 1])))
        for W in windows:
            T[a - 1] = other(vals, P[0])
            T[a:a + len(W)] = W
            ends.append(a + len(W) - 1)
            a += gap
    ends = np.array(ends, dtype=np.uint64)
    accepts = byte_accepts(P)
    D = edit_row(m, accepts, T)
    assert (D[ends.astype(np.int64)] <= 1).all()  # (the inputs, by the edit calls' oracle alone)
    with PackedText.upload(T) as pt:
        starts, dist, ops = check(P, accepts, T, pt, 1, ends, what=(vals, m))
    assert np.array_equal(dist, D[ends.astype(np.int64)].astype(np.uint8))
    kinds = set()
    for s, e, d, row in zip(starts.tolist(), ends.tolist(), dist.tolist(), ops):
        seq = unpack_ops(row)
        assert replay(seq, m, accepts, T, s, e) == d == sum(seq.count(x) for x in (SUB, INS, DEL)), (vals, m, e)
        kinds |= set(seq)
    assert kinds == {EQ, SUB, INS, DEL}


# ---- 4. the list's shape ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(20, 2), (40, 3)])
def test_the_shape_of_the_list(m, k):
    """1, 63, 64, 65, 257 and 20 000 ends from one text, shuffled, with duplicates: entry for entry what the sorted unique
    run gives; ops=False gives the same starts and distances (check)."""
    n = 16384 + 5
    rng = np.random.default_rng(2400 + m)
    P = random_text(ACGT, m, 2300 + m)
    T = np.resize(P, n)  # the pattern over and over, one symbol in 25 changed: hundreds of occurrences
    flip = rng.integers(0, 25, n) == 0
    T[flip] = np.asarray(ACGT, dtype=np.uint8)[rng.integers(0, 4, int(flip.sum()))]
    with PackedText.upload(T) as pt:
        all_ends, _, cnt = pfind_edit(P, pt, k, cap=n)
        assert cnt >= 257
        base = dict()
        s0, d0, o0 = check(P, byte_accepts(P), T, pt, k, all_ends, what=(m, k, "sorted"))
        for x, e in enumerate(all_ends.tolist()):
            base[e] = (int(s0[x]), int(d0[x]), o0[x].tolist())
        for count in (1, 63, 64, 65, 257, 20000):
            ends = all_ends[rng.integers(0, len(all_ends), count)]  # shuffled, duplicates included
            if count >= 257:
                assert len(np.unique(ends)) < count and (np.diff(ends.astype(np.int64)) < 0).any()
            starts, dist, ops = palign_edit(P, pt, k, ends)
            for x, e in enumerate(ends.tolist()):
                assert (int(starts[x]), int(dist[x]), ops[x].tolist()) == base[e], (m, k, count, x, e)
            s2, d2, o2 = palign_edit(P, pt, k, ends, ops=False)
            assert o2 is None and np.array_equal(s2, starts) and np.array_equal(d2, dist)
        # count == 0: empty arrays, no launch
        starts, dist, ops = palign_edit(P, pt, k, np.zeros(0, dtype=np.uint64))
        assert len(starts) == 0 and len(dist) == 0 and ops.shape == (0, 3)


def test_a_list_longer_than_one_piece():
    """With ops a piece of the device's buffer holds 2 Mi occurrences: 2 Mi + 77 ends (the same few hundred, repeated) go
    through two pieces and come back entry for entry."""
    n, m, k = 4097, 12, 2
    T = random_text(ACGT, n, 2500)
    P = T[1000:1000 + m].copy()
    with PackedText.upload(T) as pt:
        uniq = np.arange(n, dtype=np.uint64)  # occurrences and non-occurrences alike
        wstarts, wdist, wops = align_many(m, byte_accepts(P), T, uniq, k)
        assert (wdist != NONE_DIST).any() and (wdist == NONE_DIST).any()
        count = (2 << 20) + 77
        idx = (np.arange(count, dtype=np.int64) * 2654435761) % n
        starts, dist, ops = palign_edit(P, pt, k, uniq[idx])
        assert np.array_equal(starts, wstarts[idx]) and np.array_equal(dist, wdist[idx]) and np.array_equal(ops, wops[idx])


# ---- 5. non-occurrences ------------------------------------------------------------------------------------------------------

def test_ends_that_are_no_occurrence_get_the_sentinel():
    n, m, k = 4097, 24, 2
    T = random_text(ACGT, n, 2600)
    T[508] = other(ACGT, T[507])  # (so that the skipped symbol cannot slide: P[7] != P[8])
    P = T[500:500 + m].copy()
    T[2000:2000 + m - 1] = np.delete(P, 7)
    D = edit_row(m, byte_accepts(P), T)
    ends = np.arange(480, 2100, dtype=np.uint64)  # the two occurrences' neighbourhoods and the desert between them
    with PackedText.upload(T) as pt:
        starts, dist, ops = check(P, byte_accepts(P), T, pt, k, ends, what="sentinel")
    far = D[480:2100] > k
    assert far.sum() > 1000 and (~far).sum() >= 2
    assert (starts[far] == NONE_START).all() and (dist[far] == NONE_DIST).all() and not ops[far].any()
    assert np.array_equal(dist[~far], D[480:2100][~far].astype(np.uint8)) and (starts[~far] != NONE_START).all()
    x = 500 + m - 1 - 480
    assert (int(starts[x]), int(dist[x]), edit_cigar(ops[x])) == (500, 0, "%d=" % m)
    x = 2000 + m - 2 - 480
    assert (int(starts[x]), int(dist[x]), edit_cigar(ops[x]), edit_cigar(ops[x], sam=True)) == (2000, 1, "7=1D16=", "7=1I16=")


# ---- 6. set patterns -----------------------------------------------------------------------------------------------------------

def test_set_patterns():
    """An IUPAC primer with N, a two-member set and — by hand — an empty set, k = 2, against the oracle with set_accepts;
    singleton sets equal the byte-pattern call."""
    n = 2**14 + 5
    motif = "GGNCCWRTATAWAW"
    T = random_text(ACGT, n, 2700)
    inst = np.frombuffer(motif.replace("N", "C").replace("W", "A").replace("R", "G").encode(), dtype=np.uint8)
    T[3000:3000 + len(inst)] = inst
    T[8000:8000 + len(inst) - 1] = np.delete(inst, 5)
    T[12000:12000 + len(inst) + 1] = np.insert(inst, 3, other(ACGT, inst[2]))
    with PackedText.upload(T) as pt:
        sets = pt.iupac(motif)
        sets[9] = 0  # an empty set: it accepts nothing, every alignment pays for it
        accepts = set_accepts(sets, ACGT)
        ends, fdist, cnt = pfind_sets_edit(sets, pt, 2, cap=n)
        assert cnt >= 3 and {3000 + len(inst) - 1, 8000 + len(inst) - 2, 12000 + len(inst)} <= set(ends.tolist())
        starts, dist, ops = check(sets, accepts, T, pt, 2, ends, what="iupac", sets=True)
        assert np.array_equal(dist, fdist)
        for s, e, d, row in zip(starts.tolist(), ends.tolist(), dist.tolist(), ops):
            assert replay(unpack_ops(row), len(sets), accepts, T, s, e) == d
        P = T[5000:5000 + 40].copy()
        P[20] = other(ACGT, P[20])
        single = np.array([1 << ACGT.index(b) for b in P.tolist()], dtype=np.uint8)
        ends, _, cnt = pfind_edit(P, pt, 3, cap=n)
        assert cnt >= 1
        a, b = palign_edit(P, pt, 3, ends), palign_sets_edit(single, pt, 3, ends)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 7. a dense case -------------------------------------------------------------------------------------------------------------

def test_a_dense_case():
    """2^20 + 3 symbols on two values, m = 33, k = 7: nearly every end is an occurrence.  All ends of the find go through the
    align call; a fixed random sample of 4096 entries and the first and last 128 are compared with the oracle."""
    n, m, k = 2**20 + 3, 33, 7
    T = np.where(np.random.default_rng(2800).integers(0, 16, n) == 0, 255, 0).astype(np.uint8)  # one symbol in 16 is the other value
    P = T[77777:77777 + m].copy()
    with PackedText.upload(T) as pt:
        starts, ends, dist, ops, cnt = pfind_edit_align(P, pt, k, cap=n)
        assert cnt == len(ends) > n // 2
        s2, d2, o2 = palign_edit(P, pt, k, ends, ops=False)
        assert o2 is None and np.array_equal(s2, starts) and np.array_equal(d2, dist)
    pick = np.unique(np.concatenate([np.arange(128), np.arange(cnt - 128, cnt), np.random.default_rng(2900).integers(0, cnt, 4096)]))
    wstarts, wdist, wops = align_many(m, byte_accepts(P), T, ends[pick], k)
    assert np.array_equal(starts[pick], wstarts) and np.array_equal(dist[pick], wdist) and np.array_equal(ops[pick], wops)
    assert (starts <= ends + np.uint64(1)).all() and (dist <= k).all() and ((ops[:, 2] >> np.uint64(56)) <= m + k).all()


# ---- 8. refusals with a real text ----------------------------------------------------------------------------------------------

def test_an_end_outside_the_range_is_refused_and_names_its_index():
    T = random_text(ACGT, 1000, 3000)
    P = T[10:18].copy()
    L = smart_amd.lib()
    with PackedText.upload(T) as pt:
        for off, n, bad in ((100, 200, 99), (100, 200, 300), (0, 1000, 1000), (0, 1000, 2**63)):
            ends = np.array([150, 160, bad, 170], dtype=np.uint64)
            starts = np.full(4, 77, dtype=np.uint64)
            dist = np.full(4, 7, dtype=np.uint8)
            ops = np.full(12, 5, dtype=np.uint64)
            rc = L.smartgpu_palign_edit64(P.ctypes.data, 8, 1, pt._h, off, n, ends.ctypes.data, 4, starts.ctypes.data, dist.ctypes.data, ops.ctypes.data)
            msg = L.smartgpu_last_error().decode()
            assert rc == -3 and "ends[2] = %d" % bad in msg, (rc, msg)
            assert (starts == 77).all() and (dist == 7).all() and (ops == 5).all()  # nothing written
            with pytest.raises(smart_amd.SmartGpuError) as e:
                palign_edit(P, pt, 1, ends, off=off, n=n)
            assert "rc=-3" in str(e.value) and "ends[2]" in str(e.value)
        with pytest.raises(smart_amd.SmartGpuError):
            palign_edit(P, pt, 1, np.array([5], dtype=np.uint64), off=990, n=11)  # a range outside the text
        sets = np.array([1, 2, 16, 1], dtype=np.uint8)
        with pytest.raises(smart_amd.SmartGpuError) as e:
            palign_sets_edit(sets, pt, 1, np.array([5], dtype=np.uint64))
        assert "position 2" in str(e.value)
        # distances NULL, ops given: legal
        ends = np.array([17], dtype=np.uint64)
        starts = np.zeros(1, dtype=np.uint64)
        ops = np.zeros(3, dtype=np.uint64)
        assert L.smartgpu_palign_edit64(P.ctypes.data, 8, 1, pt._h, 0, 1000, ends.ctypes.data, 1, starts.ctypes.data, None, ops.ctypes.data) == 0
        assert starts[0] == 10 and edit_cigar(ops) == "8="
