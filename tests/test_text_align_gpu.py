"""Starts and alignments of edit-distance occurrences on BYTE texts on the GPU (smartgpu_align_edit64 and its classes form;
text_edit_align of k_talign.hip): starts, distances and operations against the DEFINITION — the plain DP of
tests/test_packed_align.py (align_many, held there to the cell-by-cell align_one) with byte_accepts / class_accepts.  Both
forms of every call are checked, with ops and without.  Every comparison is exact equality; no text here is longer than
2^14 + 5 bytes — ends beyond 2^32 are in tests/test_text_align_at_size_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (PackedText, Plan, SmartGpuError, align_edit, align_edit_classes, byte_classes, edit_cigar, engine, find_edit,  # noqa: E402
                       find_edit_align, find_edit_classes, find_edit_classes_align, palign_edit)

from test_packed_align import DEL, EQ, INS, NONE_DIST, NONE_START, SUB, align_many, replay, unpack_ops  # noqa: E402
from test_packed_edit import byte_accepts, edit_row  # noqa: E402
from test_text_align import HAND, HAND_TEXT  # noqa: E402
from test_text_edit_gpu import class_accepts, english, uploaded  # noqa: E402

ALPHABETS = {
    "two": (0, 255),
    "acgt": (65, 67, 71, 84),
    "amino": tuple(b"ACDEFGHIKLMNPQRSTVWY"),
    "all256": tuple(range(256)),
}
ALL256 = ALPHABETS["all256"]
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


def check(pat, accepts, T, text, k, ends, off=0, n=None, what=None, classes=False):
    """Both forms of the call (with and without ops) against the oracle; returns (starts, distances, ops)."""
    call = align_edit_classes if classes else align_edit
    ends = np.asarray(ends, dtype=np.uint64)
    wstarts, wdist, wops = align_many(len(pat), accepts, T, ends, k, off)
    starts, dist, ops = call(pat, text, k, ends, off=off, n=n)
    assert starts.dtype == np.uint64 and dist.dtype == np.uint8 and ops.dtype == np.uint64 and ops.shape == (len(ends), 3), what
    assert np.array_equal(starts, wstarts), (what, k, first_difference(starts, wstarts, ends))
    assert np.array_equal(dist, wdist), (what, k, first_difference(dist, wdist, ends))
    assert np.array_equal(ops, wops), (what, k, first_difference((ops != wops).any(axis=1), np.zeros(len(ends), dtype=bool), ends))
    s2, d2, o2 = call(pat, text, k, ends, off=off, n=n, ops=False)
    assert o2 is None and np.array_equal(s2, wstarts) and np.array_equal(d2, wdist), (what, k, "ops=False")
    return starts, dist, ops


def first_difference(a, b, ends):
    at = int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])
    return at, int(ends[at]), int(a[at]), int(b[at])


# ---- 1. the hand example ---------------------------------------------------------------------------------------------------

def test_the_hand_example_through_the_library():
    """tests/test_text_align.py holds the oracle to these strings; here the library is held to them."""
    T = np.frombuffer(HAND_TEXT, dtype=np.uint8)
    with uploaded(T) as text:
        for word, k, want in HAND:
            P = np.frombuffer(word, dtype=np.uint8)
            ends = np.array(sorted(want), dtype=np.uint64)
            starts, dist, ops = check(P, byte_accepts(P), T, text, k, ends, what=word)
            got = {int(e): (int(s), int(d), edit_cigar(r)) for e, s, d, r in zip(ends, starts, dist, ops)}
            assert got == want, (word, got)
            fstarts, fends, fdist, fops = find_edit_align(P, text, k)
            wends, wdist = find_edit(P, text, k)
            assert np.array_equal(fends, wends) and np.array_equal(fdist, wdist) and set(want) <= set(fends.tolist())
            wstarts, wd, wops = align_many(len(P), byte_accepts(P), T, fends, k)
            assert np.array_equal(fstarts, wstarts) and np.array_equal(fdist, wd) and np.array_equal(fops, wops), word
            found = {int(e): (int(s), int(d), edit_cigar(r)) for e, s, d, r in zip(fends, fstarts, fdist, fops)}
            assert all(found[e] == want[e] for e in want), (word, found)
        P = np.frombuffer(b"receive", dtype=np.uint8)
        _, _, ops = align_edit(P, text, 2, [12])
        assert (edit_cigar(ops[0]), edit_cigar(ops[0], sam=True)) == ("3=1D1=1D1=", "3=1I1=1I1=")


# ---- 2. lengths and alphabets ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", [1, 33, 4097])
@pytest.mark.parametrize("name", list(ALPHABETS))
def test_lengths_and_alphabets(name, n, m):
    """The pattern cut from the text (repeated where the text is shorter) and the same with one byte changed; the ends are
    the find's and so are the distances.  k = 0: every start is e - m + 1 and the operations are m times '='.  The hollow
    match s = e + 1 (k >= m) is m times 'D'."""
    vals = ALPHABETS[name]
    T = random_text(vals, n, 5000 + n + 7 * len(vals))
    mid = max(n - m, 0) // 2
    pats = [np.resize(T[mid:mid + m], m)]
    P = pats[0].copy()
    P[m // 2] = other(vals, P[m // 2])
    pats.append(P)
    hollow_seen = 0
    with uploaded(T) as text:
        for P in pats:
            for k in KS:
                ends, fdist = find_edit(P, text, k, cap=n)
                starts, dist, ops = check(P, byte_accepts(P), T, text, k, ends, what=(name, n, m))
                assert np.array_equal(dist, fdist), (name, n, m, k)  # the distances are the find's
                assert (starts <= ends + np.uint64(1)).all()
                if k == 0:
                    assert np.array_equal(starts, ends - np.uint64(m - 1)), (name, n, m)
                    assert all(unpack_ops(r) == [EQ] * m for r in ops), (name, n, m)
                hollow = starts == ends + np.uint64(1)
                assert all(unpack_ops(r) == [DEL] * m for r in ops[hollow])
                hollow_seen += int(hollow.sum())
    if m == 1 and n > 1:
        assert hollow_seen > 0  # (the inputs: the hollow match was met — every end whose byte is not the pattern's, at k >= 1)


# ---- 3. clipping and window phases -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(8, 1), (31, 3), (32, 7), (33, 0), (64, 7)])
@pytest.mark.parametrize("name", ["all256", "two"])
def test_clipping_and_window_phases(name, m, k):
    """Ranges that start at off: the ends off .. off + m + k (every walk shorter than m + k columns, down to one), every e < 80
    of the range (the window reaches below text byte 0, at every e % 4), and the last end of the text.  A copy of the pattern
    one byte after off, and one that off cuts.  No start lies below off."""
    vals = ALPHABETS[name]
    n = 4097
    T = random_text(vals, n, 5100 + m)
    P = T[2040:2040 + m].copy()
    for off in (0, 1, 2, 3, 4, 5, 75, 76, 77):
        for at in (off + 1, off - 1):
            if at < 0:
                continue
            T2 = T.copy()
            T2[at:at + m] = P
            ends = set(range(off, off + m + k + 1)) | {e for e in range(80) if e >= off} | {n - 1}
            ends = np.array(sorted(ends), dtype=np.uint64)
            with uploaded(T2) as text:
                starts, dist, _ = check(P, byte_accepts(P), T2, text, k, ends, off=off, n=n - off, what=(name, m, k, off, at))
            hit = dist != NONE_DIST
            assert (starts[hit] >= off).all() and (starts[~hit] == NONE_START).all()
            x = ends.tolist().index(at + m - 1)
            if at > off:
                assert (int(starts[x]), int(dist[x])) == (at, 0)
            elif k >= 1:
                assert int(dist[x]) <= 1 and int(starts[x]) >= off


# ---- 4. planted edits ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [40, 64])
@pytest.mark.parametrize("name", ["all256", "two"])
def test_one_planted_edit_at_every_pattern_position(name, m):
    """One substitution, one deletion and one insertion at every pattern position, all in ONE text.  Compared against the
    oracle, not the planted offset, and every operation sequence replays: '=' on accepted bytes, 'X' on others, m pattern
    bytes, e - s + 1 text bytes, X + I + D = d.  All four operations occur."""
    vals = ALPHABETS[name]
    P = random_text(vals, m, 5300 + m + len(vals))
    gap = m + 16
    n = 3 * m * gap + 64
    T = random_text(vals, n, 5400 + m)
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
    with uploaded(T) as text:
        starts, dist, ops = check(P, accepts, T, text, 1, ends, what=(name, m))
    assert np.array_equal(dist, D[ends.astype(np.int64)].astype(np.uint8))
    kinds = set()
    for s, e, d, row in zip(starts.tolist(), ends.tolist(), dist.tolist(), ops):
        seq = unpack_ops(row)
        assert replay(seq, m, accepts, T, s, e) == d == sum(seq.count(x) for x in (SUB, INS, DEL)), (name, m, e)
        kinds |= set(seq)
    assert kinds == {EQ, SUB, INS, DEL}


# ---- 5. the list's shape ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(20, 2), (40, 3)])
def test_the_shape_of_the_list(m, k):
    """1 .. 20 000 ends from one text — around one workgroup's 32 and 64 occurrences —, shuffled, with duplicates: entry for
    entry what the sorted unique run gives; ops=False gives the same starts and distances."""
    n = 16384 + 5
    rng = np.random.default_rng(5500 + m)
    P = random_text(ALPHABETS["amino"], m, 5600 + m)
    T = np.resize(P, n)  # the pattern over and over, one byte in 25 redrawn: hundreds of occurrences
    flip = rng.integers(0, 25, n) == 0
    T[flip] = np.asarray(ALPHABETS["amino"], dtype=np.uint8)[rng.integers(0, 20, int(flip.sum()))]
    with uploaded(T) as text:
        all_ends, _ = find_edit(P, text, k, cap=n)
        assert len(all_ends) >= 257
        s0, d0, o0 = check(P, byte_accepts(P), T, text, k, all_ends, what=(m, k, "sorted"))
        base = {e: (int(s0[x]), int(d0[x]), o0[x].tolist()) for x, e in enumerate(all_ends.tolist())}
        for count in (1, 31, 32, 33, 63, 64, 65, 257, 20000):
            ends = all_ends[rng.integers(0, len(all_ends), count)]  # shuffled, duplicates included
            if count >= 257:
                assert len(np.unique(ends)) < count and (np.diff(ends.astype(np.int64)) < 0).any()
            starts, dist, ops = align_edit(P, text, k, ends)
            for x, e in enumerate(ends.tolist()):
                assert (int(starts[x]), int(dist[x]), ops[x].tolist()) == base[e], (m, k, count, x, e)
            s2, d2, o2 = align_edit(P, text, k, ends, ops=False)
            assert o2 is None and np.array_equal(s2, starts) and np.array_equal(d2, dist)
        # count == 0: empty arrays, no launch
        for ops_wanted in (True, False):
            starts, dist, ops = align_edit(P, text, k, np.zeros(0, dtype=np.uint64), ops=ops_wanted)
            assert len(starts) == 0 and len(dist) == 0 and (ops.shape == (0, 3) if ops_wanted else ops is None)
        starts, dist, ops = align_edit_classes(byte_classes(P), text, k, [])
        assert len(starts) == 0 and len(dist) == 0 and ops.shape == (0, 3)


def test_a_list_longer_than_one_piece():
    """With ops a piece of the device's buffer holds 2 Mi occurrences: 2 Mi + 77 ends (the same few thousand, repeated) go
    through two pieces and come back entry for entry."""
    n, m, k = 4097, 12, 2
    T = random_text(ALPHABETS["acgt"], n, 5700)
    P = T[1000:1000 + m].copy()
    uniq = np.arange(n, dtype=np.uint64)  # occurrences and non-occurrences alike
    wstarts, wdist, wops = align_many(m, byte_accepts(P), T, uniq, k)
    assert (wdist != NONE_DIST).any() and (wdist == NONE_DIST).any()
    count = (2 << 20) + 77
    idx = (np.arange(count, dtype=np.int64) * 2654435761) % n
    with uploaded(T) as text:
        starts, dist, ops = align_edit(P, text, k, uniq[idx])
    assert np.array_equal(starts, wstarts[idx]) and np.array_equal(dist, wdist[idx]) and np.array_equal(ops, wops[idx])


# ---- 6. non-occurrences ------------------------------------------------------------------------------------------------------

def test_ends_that_are_no_occurrence_get_the_sentinel():
    n, m, k = 4097, 24, 2
    T = random_text(ALL256, n, 5800)
    T[508] = other(ALL256, T[507])  # (so that the skipped byte cannot slide: P[7] != P[8])
    P = T[500:500 + m].copy()
    T[2000:2000 + m - 1] = np.delete(P, 7)
    D = edit_row(m, byte_accepts(P), T)
    ends = np.arange(480, 2100, dtype=np.uint64)  # the two occurrences' neighbourhoods and the desert between them
    with uploaded(T) as text:
        starts, dist, ops = check(P, byte_accepts(P), T, text, k, ends, what="sentinel")
    far = D[480:2100] > k
    assert far.sum() > 1000 and (~far).sum() >= 2
    assert (starts[far] == NONE_START).all() and (dist[far] == NONE_DIST).all() and not ops[far].any()
    assert np.array_equal(dist[~far], D[480:2100][~far].astype(np.uint8)) and (starts[~far] != NONE_START).all()
    x = 500 + m - 1 - 480
    assert (int(starts[x]), int(dist[x]), edit_cigar(ops[x])) == (500, 0, "%d=" % m)
    x = 2000 + m - 2 - 480
    assert (int(starts[x]), int(dist[x]), edit_cigar(ops[x]), edit_cigar(ops[x], sam=True)) == (2000, 1, "7=1D16=", "7=1I16=")


# ---- 7. classes ----------------------------------------------------------------------------------------------------------------

def test_classes():
    """byte_classes(P, ignore_case=True) on the English excerpt against the oracle; a row emptied by hand and a full row;
    singleton rows equal the byte-pattern call."""
    E = english()[:2**14 + 5]
    fold = np.arange(256, dtype=np.uint8)
    fold[65:91] += 32
    with uploaded(E) as text:
        for word, k in ((b"aND gOD sAID", 1), (b"THE LORD", 0), (b"the lord god", 2), (b"AnD iT cAmE tO pAsS, wHeN", 3)):
            P = np.frombuffer(word, dtype=np.uint8)
            rows = byte_classes(P, ignore_case=True)
            folded = lambda i, R, P=P: fold[R] == fold[P[i]]  # noqa: E731
            starts, ends, dist, ops = find_edit_classes_align(rows, text, k, cap=len(E))
            wends, wdist = find_edit_classes(rows, text, k, cap=len(E))
            assert len(ends) >= 1 and np.array_equal(ends, wends) and np.array_equal(dist, wdist), word
            s, d, o = check(rows, folded, E, text, k, ends, what=word, classes=True)
            assert np.array_equal(s, starts) and np.array_equal(d, dist) and np.array_equal(o, ops), word
            # the same through the oracle that reads the rows themselves
            ws, wd, wo = align_many(len(P), class_accepts(rows), E, ends, k)
            assert np.array_equal(s, ws) and np.array_equal(d, wd) and np.array_equal(o, wo), word
        # rows by hand: an EMPTY row (accepts nothing: one edit at least) and a FULL row among letters
        rows = np.zeros((6, 32), dtype=np.uint8)
        for j, members in enumerate((b"tT", b"aeiou", b"", None, b" ,.;:", b"aeiouAEIOU")):
            for v in (range(256) if members is None else members):
                rows[j, v >> 3] |= 1 << (v & 7)
        assert not rows[2].any() and (rows[3] == 255).all()
        accepts = class_accepts(rows)
        for k in (1, 2):
            ends, fdist = find_edit_classes(rows, text, k, cap=len(E))
            assert len(ends) >= 1 and fdist.min() >= 1
            starts, dist, ops = check(rows, accepts, E, text, k, ends, what=("by hand", k), classes=True)
            assert np.array_equal(dist, fdist)
            for s, e, d, row in zip(starts.tolist()[:200], ends.tolist()[:200], dist.tolist()[:200], ops[:200]):
                assert replay(unpack_ops(row), 6, accepts, E, s, e) == d
        # one bit per row: the byte-pattern call
        P = E[5000:5040].copy()
        P[20] = other(ALL256, P[20])
        ends, _ = find_edit(P, text, 3, cap=len(E))
        assert len(ends) >= 1
        ends = np.concatenate([ends, np.arange(4000, 4100, dtype=np.uint64)])
        a, b = align_edit(P, text, 3, ends), align_edit_classes(byte_classes(P), text, 3, ends)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        align_edit_classes(np.zeros((4, 16), dtype=np.uint8), None, 1, [3])


# ---- 8. the packed kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["acgt", "two"])
def test_the_packed_kernel_gives_identical_arrays(name):
    """planes_edit_align is an independent kernel: the same bytes packed, the same P, k and ends."""
    vals = ALPHABETS[name]
    n = 2**14 + 5
    T = random_text(vals, n, 5900 + len(vals))
    rng = np.random.default_rng(6000)
    with uploaded(T) as text:
        pt = PackedText.pack(text)
        try:
            for m, k in ((12, 1), (20, 3), (33, 7), (64, 7)):
                P = T[5000:5000 + m].copy()
                for off, ln in ((0, n), (129, 9000), (4001, n - 4001)):  # (the pattern's own place lies in each)
                    ends, _ = find_edit(P, text, k, off=off, n=ln, cap=n)
                    assert len(ends) >= 1
                    ends = np.concatenate([ends[:3000], (off + rng.integers(0, ln, 500)).astype(np.uint64)])
                    for ops in (True, False):
                        a = align_edit(P, text, k, ends, off=off, n=ln, ops=ops)
                        b = palign_edit(P, pt, k, ends, off=off, n=ln, ops=ops)
                        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, m, k, off)
                        assert (a[2] is None and b[2] is None) if not ops else np.array_equal(a[2], b[2]), (name, m, k, off)
        finally:
            pt.free()


# ---- 9. refusals with a real text ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["", "_classes"])
def test_refusals_with_a_real_text(kind):
    T = random_text(ALPHABETS["amino"], 1000, 6100)
    P = T[10:18].copy()
    pat = byte_classes(P) if kind else P
    L = smart_amd.lib()
    f = getattr(L, "smartgpu_align_edit%s64" % kind)
    call = align_edit_classes if kind else align_edit
    with uploaded(T) as text:
        for off, n, bad in ((100, 200, 99), (100, 200, 300), (0, 1000, 1000), (0, 1000, 2**63)):
            ends = np.array([150, 160, bad, 170], dtype=np.uint64)
            starts = np.full(4, 77, dtype=np.uint64)
            dist = np.full(4, 7, dtype=np.uint8)
            ops = np.full(12, 5, dtype=np.uint64)
            rc = f(pat.ctypes.data, 8, 1, text._h, off, n, ends.ctypes.data, 4, starts.ctypes.data, dist.ctypes.data, ops.ctypes.data)
            msg = L.smartgpu_last_error().decode()
            assert rc == -3 and "ends[2] = %d" % bad in msg, (rc, msg)
            assert (starts == 77).all() and (dist == 7).all() and (ops == 5).all()  # nothing written
            with pytest.raises(SmartGpuError) as e:
                call(pat, text, 1, ends, off=off, n=n)
            assert "rc=-3" in str(e.value) and "ends[2]" in str(e.value)
        # a range outside the text
        starts = np.full(1, 77, dtype=np.uint64)
        ends = np.array([995], dtype=np.uint64)
        assert f(pat.ctypes.data, 8, 1, text._h, 990, 11, ends.ctypes.data, 1, starts.ctypes.data, None, None) == -3 and starts[0] == 77
        assert "outside the text" in L.smartgpu_last_error().decode()
        with pytest.raises(SmartGpuError):
            call(pat, text, 1, ends, off=990, n=11)
        # count == 0 with a valid text: SMARTGPU_OK, NULL lists
        assert f(pat.ctypes.data, 8, 1, text._h, 0, 1000, None, 0, None, None, None) == 0
        # distances NULL, ops given: legal
        ends = np.array([17], dtype=np.uint64)
        starts = np.zeros(1, dtype=np.uint64)
        ops = np.zeros(3, dtype=np.uint64)
        assert f(pat.ctypes.data, 8, 1, text._h, 0, 1000, ends.ctypes.data, 1, starts.ctypes.data, None, ops.ctypes.data) == 0
        assert starts[0] == 10 and edit_cigar(ops) == "8="
        # more than cap occurrences: the find's refusal
        with pytest.raises(SmartGpuError, match="occurrences"):
            (find_edit_classes_align if kind else find_edit_align)(pat, text, 7, cap=5)


# ---- 10. the coalescing queue ----------------------------------------------------------------------------------------------------

def test_a_call_behind_queued_horspool_launches():
    """Plan.launch calls wait in the coalescing queue; an align call on the same text sends them first (device_ctx_flushed) and
    never enters the queue itself.  Both give their right answers."""
    from test_coalesce_gpu import cut
    rng = np.random.default_rng(6200)
    n = 3 * 32768 + 99
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
    T[70000:70019] = np.delete(Q, 9)
    raw = T.tobytes()
    ends = np.array([20019, 70018, 70017, 30000], dtype=np.uint64)
    want = align_many(20, byte_accepts(Q), T, ends, 2)
    assert want[1].tolist()[:2] == [0, 1] and want[1][3] == NONE_DIST
    default = engine.coalesce(8)
    try:
        with uploaded(T) as text:
            plans = [Plan("hor", P) for P in pats]
            try:
                engine.device_sync(0)
                l0, p0 = engine.coalesce_stats(0)
                for pl in plans:
                    pl.launch(text)
                got = align_edit(Q, text, 2, ends)  # the queue is sent here
                engine.device_sync(0)
                l1, p1 = engine.coalesce_stats(0)
                assert all(np.array_equal(x, y) for x, y in zip(got, want))
                assert [pl.result(0)[0] for pl in plans] == [occurrences(P) for P in pats]
                assert (l1 - l0, p1 - p0) == (len(plans), 1)  # the four launches were queued, and left as ONE pass
            finally:
                for pl in plans:
                    pl.free()
    finally:
        engine.device_sync(0)
        engine.coalesce(default)


# ---- 11. a seeded differential fuzz ------------------------------------------------------------------------------------------------

FUZZ_CASES, FUZZ_PARTS = 300, 4


def fuzz_case(rng):
    """(T, pat, accepts, classes?, k, off, n, ops?): a text of at most 5000 bytes, a range that begins and ends anywhere — mid-dword
    mostly —, a pattern cut from the range with up to k + 1 edits, as bytes or as classes with extra members, an empty or a
    full row now and then."""
    vals = list(ALPHABETS.values())[int(rng.integers(0, 4))]
    total = int(rng.integers(1, 5001))
    T = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), total)]
    off = int(rng.integers(0, total))
    n = int(rng.integers(1, total - off + 1))
    m = int(rng.choice([1, 2, 3, 8, 20, 31, 32, 33, 40, 63, 64]))
    k = int(rng.integers(0, 8))
    a = off + int(rng.integers(0, n))
    W = [int(x) for x in np.resize(T[a:a + m], m)]
    for _ in range(int(rng.integers(0, k + 2))):
        j = int(rng.integers(0, len(W)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            W[j] = int(vals[int(rng.integers(0, len(vals)))])
        elif kind == 1 and len(W) > 1:
            del W[j]
        elif len(W) < 64:
            W.insert(j, int(vals[int(rng.integers(0, len(vals)))]))
    P = np.asarray(W, dtype=np.uint8)
    if rng.integers(0, 2) == 0:
        return T, P, byte_accepts(P), False, k, off, n, bool(rng.integers(0, 2))
    rows = byte_classes(P)
    for j in range(len(P)):
        for _ in range(int(rng.integers(0, 3))):
            v = int(vals[int(rng.integers(0, len(vals)))])
            rows[j, v >> 3] |= 1 << (v & 7)
    if rng.integers(0, 4) == 0:
        rows[int(rng.integers(0, len(P)))] = 0
    if rng.integers(0, 4) == 0:
        rows[int(rng.integers(0, len(P)))] = 255
    return T, rows, class_accepts(rows), True, k, off, n, bool(rng.integers(0, 2))


@pytest.mark.parametrize("part", range(FUZZ_PARTS))
def test_seeded_differential_fuzz(part):
    """300 cases in four parts.  The ends are a random mix of the find's and arbitrary ones of the range, shuffled; the case index
    is in every assertion message."""
    per = FUZZ_CASES // FUZZ_PARTS
    hits = misses = 0
    for case in range(part * per, (part + 1) * per):
        rng = np.random.default_rng(70000 + case)
        T, pat, accepts, classes, k, off, n, ops = fuzz_case(rng)
        find = find_edit_classes if classes else find_edit
        call = align_edit_classes if classes else align_edit
        with uploaded(T) as text:
            fends, fdist = find(pat, text, k, off=off, n=n, cap=n)
            mine = fends[rng.integers(0, len(fends), min(len(fends), 48))] if len(fends) else fends
            ends = np.concatenate([mine, (off + rng.integers(0, n, 24)).astype(np.uint64)])
            rng.shuffle(ends)
            starts, dist, words = call(pat, text, k, ends, off=off, n=n, ops=ops)
        wstarts, wdist, wwords = align_many(len(pat), accepts, T, ends, k, off)
        what = ("case", case, "classes" if classes else "bytes", len(pat), k, off, n, ops)
        assert np.array_equal(starts, wstarts), (what, first_difference(starts, wstarts, ends))
        assert np.array_equal(dist, wdist), (what, first_difference(dist, wdist, ends))
        assert (words is None) if not ops else np.array_equal(words, wwords), what
        # the find's distances at the find's ends
        lookup = dict(zip(fends.tolist(), fdist.tolist()))
        assert all(lookup.get(e, NONE_DIST) == d for e, d in zip(ends.tolist(), dist.tolist())), what
        assert (starts[dist != NONE_DIST] >= off).all(), what
        hits += int((dist != NONE_DIST).sum())
        misses += int((dist == NONE_DIST).sum())
    assert hits > per and misses > per  # (the inputs: both kinds of end in number)
