"""Starts and alignments of LONG edit-distance occurrences on byte texts on the GPU (smartgpu_align_editl64 and its classes
form; text_editl_align of k_talignl.hip: m <= 256, k <= 31, ten words of operations per entry): starts, distances and
operations against the DEFINITION — the ten-word vector oracle of tests/test_text_alignl.py (align_manyl, held there to the
cell-by-cell align_one of tests/test_packed_align.py).  Both forms of every call are checked, with ops and without.  Every
comparison is exact equality.  The kernel's unit of work is one occurrence, so texts of a few KiB reach every path; ends
beyond 2^32 are in tests/test_text_alignl_at_size_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (Plan, SmartGpuError, align_edit, align_editl, align_editl_classes, byte_classes, edit_cigar, engine, find_editl,  # noqa: E402
                       find_editl_align, find_editl_classes, find_editl_classes_align)

from test_packed_align import DEL, EQ, INS, NONE_DIST, NONE_START, SUB, replay, unpack_ops  # noqa: E402
from test_packed_edit import byte_accepts  # noqa: E402
from test_text_alignl import WORDS, align_manyl, unpack_opsl  # noqa: E402
from test_text_edit_gpu import class_accepts, english, uploaded  # noqa: E402

TEXTS = {"one": (97,), "acgt": (65, 67, 71, 84), "rand128": tuple(range(128)), "english": None}
MS = [1, 31, 32, 33, 64, 65, 100, 128, 129, 200, 255, 256]
KS = [0, 3, 7, 8, 15, 31]
PIECE_WITH_OPS = (8 << 20) // (1 + WORDS)  # occurrences of one piece of the device's find buffer (host_ctx.hpp: kFindKeep)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def draw_text(name, n, seed):
    if name == "english":
        return english()[1000:1000 + n].copy()
    vals = TEXTS[name]
    return np.asarray(vals, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(vals), n)]


def other(v):
    return (int(v) + 1) % 128 if v != 97 else 98


def mixed_edits(P, d, rng, vals):
    """P with d edits of the three kinds in turn at distinct places, kept apart where the pattern has the room."""
    W = [int(x) for x in P]
    if d == 0 or len(W) < 3:
        return np.asarray(W, dtype=np.uint8)
    places = sorted(rng.choice(np.arange(1, len(W) - 1), size=min(d, len(W) - 2), replace=False).tolist(), reverse=True)
    for t, j in enumerate(places):
        v = int(vals[int(rng.integers(0, len(vals)))])
        if t % 3 == 0:
            W[j] = v if v != W[j] else int(vals[(list(vals).index(v) + 1) % len(vals)])
        elif t % 3 == 1:
            del W[j]
        else:
            W.insert(j, v)
    return np.asarray(W, dtype=np.uint8)


def first_difference(a, b, ends):
    at = int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])
    return at, int(ends[at]), int(a[at]), int(b[at])


def check(pat, accepts, T, text, k, ends, off=0, n=None, what=None, classes=False):
    """Both forms of the call (with and without ops) against the oracle, and every hit replayed; returns (starts, distances, ops)."""
    call = align_editl_classes if classes else align_editl
    ends = np.asarray(ends, dtype=np.uint64)
    m = len(pat)
    wstarts, wdist, wops = align_manyl(m, accepts, T, ends, k, off)
    starts, dist, ops = call(pat, text, k, ends, off=off, n=n)
    assert starts.dtype == np.uint64 and dist.dtype == np.uint8 and ops.dtype == np.uint64 and ops.shape == (len(ends), WORDS), what
    assert np.array_equal(dist, wdist), (what, k, first_difference(dist, wdist, ends))
    assert np.array_equal(starts, wstarts), (what, k, first_difference(starts, wstarts, ends))
    assert np.array_equal(ops, wops), (what, k, first_difference((ops != wops).any(axis=1), np.zeros(len(ends), dtype=bool), ends))
    s2, d2, o2 = call(pat, text, k, ends, off=off, n=n, ops=False)
    assert o2 is None and np.array_equal(s2, wstarts) and np.array_equal(d2, wdist), (what, k, "ops=False")
    for s, e, d, row in zip(starts.tolist(), ends.tolist(), dist.tolist(), ops):
        if d == NONE_DIST:
            assert s == int(NONE_START) and not row.any(), (what, k, e)
        else:
            assert d <= min(k, 31) and off <= s <= e + 1 and replay(unpack_opsl(row), m, accepts, T, s, e) == d, (what, k, e)
    return starts, dist, ops


# ---- 1. lengths and alphabets ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", list(TEXTS))
def test_lengths_and_alphabets(name, m):
    """A pattern cut from the text with three mixed edits, at every k: the ends are the find's (a seeded sample where there are
    many) and so are the distances, plus a seeded sample of arbitrary ends, which on the larger alphabets are no occurrences
    and get the sentinel.  k = 0 on the exact pattern: every start is e - m + 1 and the operations are m times '='."""
    n = 3001
    T = draw_text(name, n, 7000 + m)
    vals = np.unique(T)
    rng = np.random.default_rng(7100 + m)
    exact = T[1500:1500 + m].copy()
    P = mixed_edits(exact, 3, rng, vals)
    hits = misses = 0
    with uploaded(T) as text:
        for k in KS:
            for pat in (exact, P) if k in (0, 31) else (P,):
                fends, fdist = find_editl(pat, text, k, cap=n)
                pick = np.sort(rng.choice(len(fends), size=min(len(fends), 96), replace=False)) if len(fends) else np.zeros(0, dtype=np.int64)
                ends = np.concatenate([fends[pick], rng.integers(0, n, 48).astype(np.uint64), np.array([1500 + m - 1], dtype=np.uint64)])
                starts, dist, ops = check(pat, byte_accepts(pat), T, text, k, ends, what=(name, m))
                assert np.array_equal(dist[:len(pick)], fdist[pick]), (name, m, k)  # the distances are the find's
                lookup = dict(zip(fends.tolist(), fdist.tolist()))
                assert all(lookup.get(e, NONE_DIST) == d for e, d in zip(ends.tolist(), dist.tolist())), (name, m, k)
                hits += int((dist != NONE_DIST).sum())
                misses += int((dist == NONE_DIST).sum())
                if k == 0 and pat is exact:
                    at = ends.tolist().index(1500 + m - 1)
                    assert int(starts[at]) == 1500 and unpack_opsl(ops[at]) == [EQ] * m, (name, m)
                    hit = dist == 0
                    assert np.array_equal(starts[hit], ends[hit] - np.uint64(m - 1)), (name, m)
    assert hits > 0 and (misses > 0 or name == "one" or m == 1)  # (the inputs: both kinds of end)


# ---- 2. clipping and window phases ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(33, 0), (65, 8), (100, 15), (200, 7), (256, 31)])
@pytest.mark.parametrize("name", ["rand128", "acgt"])
def test_clipping_and_window_phases(name, m, k):
    """A range that starts at off = 129: the ends off .. off + m + k + 2 (every band narrower than m + k columns, down to one,
    then the first full ones; every e % 4).  A range that starts at 0: every e < 4 * 72 + 3, whose windows reach into the pad
    below text byte 0.  The last byte of the text.  A copy of the pattern one byte after off, and one that off cuts.  No
    start lies below off."""
    n = 2049
    T = draw_text(name, n, 7200 + m)
    P = T[1200:1200 + m].copy()
    for off, at in ((129, 130), (129, 128), (0, 1), (0, 0)):
        T2 = T.copy()
        T2[at:at + m] = P
        T2[n - m:] = P  # an occurrence that ends with the text's last byte
        ends = set(range(off, min(off + m + k + 3, n))) | {n - 1}
        if off == 0:
            ends |= set(range(0, 4 * 72 + 3))
        ends = np.array(sorted(ends), dtype=np.uint64)
        with uploaded(T2) as text:
            starts, dist, _ = check(P, byte_accepts(P), T2, text, k, ends, off=off, n=n - off, what=(name, m, k, off, at))
        hit = dist != NONE_DIST
        assert (starts[hit] >= off).all() and (starts[~hit] == NONE_START).all()
        assert (int(starts[-1]), int(dist[-1])) == (n - m, 0)
        x = ends.tolist().index(at + m - 1)
        if at >= off:
            assert (int(starts[x]), int(dist[x])) == (at, 0)
        elif k >= 1:
            assert int(dist[x]) <= 1 and int(starts[x]) >= off


# ---- 3. planted edits ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rand128", "acgt"])
def test_one_planted_edit_of_each_kind_at_every_pattern_position(name):
    """m = 100, k = 2: one substitution, one deletion and one insertion at every pattern position, all in ONE text.  Compared
    against the oracle, not the planted offset, and every operation sequence replays (check).  All four operations occur."""
    m, k = 100, 2
    vals = TEXTS[name]
    P = draw_text(name, m, 7300)
    gap = m + 12
    n = 3 * m * gap + 64
    T = draw_text(name, n, 7301)
    alt = lambda v: int(vals[(vals.index(int(v)) + 1) % len(vals)])  # noqa: E731
    ends, a = [], 8
    for j in range(m):
        sub = P.copy()
        sub[j] = alt(sub[j])
        windows = [sub, np.delete(P, j)]
        if j > 0:
            windows.append(np.insert(P, j, alt(P[j - 1])))
        for W in windows:
            T[a - 1] = alt(P[0])
            T[a:a + len(W)] = W
            ends.append(a + len(W) - 1)
            a += gap
    ends = np.array(ends, dtype=np.uint64)
    with uploaded(T) as text:
        starts, dist, ops = check(P, byte_accepts(P), T, text, k, ends, what=(name, m))
    assert (dist <= 1).all()
    kinds = set()
    for row in ops:
        kinds |= set(unpack_opsl(row))
    assert kinds == {EQ, SUB, INS, DEL}


def test_a_planted_copy_with_exactly_31_mixed_edits_at_m_256():
    """Over 128 values 31 edits kept apart cannot be explained by fewer: D(e) = 31, the largest distance the call reports; the
    same copy is no occurrence at k = 30."""
    m = 256
    rng = np.random.default_rng(7400)
    T = draw_text("rand128", 4097, 7401)
    P = draw_text("rand128", m, 7402)
    W = [int(x) for x in P]
    places = list(range(4, 4 + 31 * 8, 8))[::-1]  # 31 places, eight apart
    for t, j in enumerate(places):
        if t % 3 == 0:
            W[j] = other(W[j])
        elif t % 3 == 1:
            del W[j]
        else:
            W.insert(j, other(W[j - 1]))
    W = np.asarray(W, dtype=np.uint8)
    T[2000:2000 + len(W)] = W
    e = 2000 + len(W) - 1
    ends = np.arange(e - 40, e + 41, dtype=np.uint64)
    with uploaded(T) as text:
        starts, dist, ops = check(P, byte_accepts(P), T, text, 31, ends, what="31 edits")
        x = 40
        assert (int(starts[x]), int(dist[x])) == (2000, 31)
        seq = unpack_opsl(ops[x])
        assert len(seq) == int(ops[x][WORDS - 1]) and sum(seq.count(o) for o in (SUB, INS, DEL)) == 31 and {SUB, INS, DEL} <= set(seq)
        fends, fdist = find_editl(P, text, 31)
        assert e in fends.tolist() and int(fdist[fends.tolist().index(e)]) == 31
        s30, d30, o30 = check(P, byte_accepts(P), T, text, 30, ends[x:x + 1], what="30 edits")
        assert d30[0] == NONE_DIST and not o30.any()
        rng.shuffle(ends)  # and the same ends in another order
        check(P, byte_accepts(P), T, text, 31, ends, what="31 edits, shuffled")


# ---- 4. the short kernel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["acgt", "rand128", "english"])
def test_the_short_call_gives_the_same_answers(name):
    """For m <= 64, k <= 7 text_edit_align (smartgpu_align_edit64) is an independent kernel: the same starts and distances on
    the same ends, and the same operations once both packings are unpacked."""
    n = 2**13 + 5
    T = draw_text(name, n, 7500)
    rng = np.random.default_rng(7501)
    with uploaded(T) as text:
        for m, k in ((1, 1), (12, 1), (20, 3), (32, 7), (33, 0), (64, 7)):
            P = mixed_edits(T[3000:3000 + m], min(k, 2), rng, np.unique(T))
            for off, ln in ((0, n), (129, 5000)):
                fends, _ = find_editl(P, text, k, off=off, n=ln, cap=n)
                assert len(fends) >= 1
                ends = np.concatenate([fends[:1500], (off + rng.integers(0, ln, 300)).astype(np.uint64)])
                a = align_editl(P, text, k, ends, off=off, n=ln)
                b = align_edit(P, text, k, ends, off=off, n=ln)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, m, k, off)
                assert all(unpack_opsl(x) == unpack_ops(y) for x, y in zip(a[2], b[2])), (name, m, k, off)
                a2, b2 = align_editl(P, text, k, ends, off=off, n=ln, ops=False), align_edit(P, text, k, ends, off=off, n=ln, ops=False)
                assert a2[2] is None and np.array_equal(a2[0], b2[0]) and np.array_equal(a2[1], b2[1]), (name, m, k, off)


# ---- 5. classes --------------------------------------------------------------------------------------------------------------------

def test_classes():
    """byte_classes(P, ignore_case=True) on the English excerpt against the oracle; a row emptied by hand and a full row;
    one-bit rows equal the byte-pattern call."""
    E = english()[:2**13 + 5]
    fold = np.arange(256, dtype=np.uint8)
    fold[65:91] += 32
    with uploaded(E) as text:
        sentence = E[4000:4000 + 130].copy()
        for word, k in ((b"aND gOD sAID", 1), (sentence.tobytes().swapcase(), 9), (sentence[:70].tobytes().upper(), 0)):
            P = np.frombuffer(word, dtype=np.uint8)
            rows = byte_classes(P, ignore_case=True)
            folded = lambda i, R, P=P: fold[R] == fold[P[i]]  # noqa: E731
            starts, ends, dist, ops = find_editl_classes_align(rows, text, k, cap=len(E))
            wends, wdist = find_editl_classes(rows, text, k, cap=len(E))
            assert len(ends) >= 1 and np.array_equal(ends, wends) and np.array_equal(dist, wdist), word
            s, d, o = check(rows, folded, E, text, k, ends, what=word, classes=True)
            assert np.array_equal(s, starts) and np.array_equal(d, dist) and np.array_equal(o, ops), word
            ws, wd, wo = align_manyl(len(P), class_accepts(rows), E, ends, k)  # the oracle that reads the rows themselves
            assert np.array_equal(s, ws) and np.array_equal(d, wd) and np.array_equal(o, wo), word
        # rows by hand: an EMPTY row (accepts nothing: one edit at least) and a FULL row among the sentence's letters
        rows = byte_classes(sentence)
        rows[40] = 0
        rows[90] = 255
        accepts = class_accepts(rows)
        for k in (1, 12):
            ends, fdist = find_editl_classes(rows, text, k, cap=len(E))
            assert len(ends) >= 1 and fdist.min() >= 1
            starts, dist, ops = check(rows, accepts, E, text, k, ends, what=("by hand", k), classes=True)
            assert np.array_equal(dist, fdist)
        # one bit per row: the byte-pattern call
        P = sentence.copy()
        P[20] = other(P[20])
        ends, _ = find_editl(P, text, 3, cap=len(E))
        assert len(ends) >= 1
        ends = np.concatenate([ends, np.arange(3900, 4200, dtype=np.uint64)])
        a, b = align_editl(P, text, 3, ends), align_editl_classes(byte_classes(P), text, 3, ends)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        align_editl_classes(np.zeros((4, 16), dtype=np.uint8), None, 1, [3])


# ---- 6. the list's shape -----------------------------------------------------------------------------------------------------------

def test_the_shape_of_the_list():
    """Duplicates, descending order, count = 1 and count = 0 — and counts around the four waves of a workgroup — from one text:
    entry for entry what the sorted unique run gives."""
    m, k, n = 100, 3, 8192 + 5
    rng = np.random.default_rng(7600)
    P = draw_text("rand128", m, 7601)
    T = draw_text("rand128", n, 7602)
    for t, a in enumerate(range(20, n - 2 * m, 130)):  # a copy with 0 .. 3 mixed edits every 130 bytes
        W = mixed_edits(P, t % 4, rng, np.arange(128))
        T[a:a + len(W)] = W
    with uploaded(T) as text:
        all_ends, _ = find_editl(P, text, k, cap=n)
        assert len(all_ends) >= 40
        all_ends = np.concatenate([all_ends[:120], np.arange(5000, 5040, dtype=np.uint64)])
        s0, d0, o0 = check(P, byte_accepts(P), T, text, k, all_ends, what="sorted")
        assert (d0 != NONE_DIST).any() and (d0 == NONE_DIST).any()
        base = {e: (int(s0[x]), int(d0[x]), o0[x].tolist()) for x, e in enumerate(all_ends.tolist())}
        for count in (1, 3, 4, 5, 257, 5000):
            ends = all_ends[rng.integers(0, len(all_ends), count)]  # shuffled, duplicates included
            if count >= 257:
                assert len(np.unique(ends)) < count
            for order in (ends, np.sort(ends)[::-1].copy()):  # as drawn, and descending
                starts, dist, ops = align_editl(P, text, k, order)
                for x, e in enumerate(order.tolist()):
                    assert (int(starts[x]), int(dist[x]), ops[x].tolist()) == base[e], (count, x, e)
                s2, d2, o2 = align_editl(P, text, k, order, ops=False)
                assert o2 is None and np.array_equal(s2, starts) and np.array_equal(d2, dist)
        for ops_wanted in (True, False):  # count == 0: empty arrays, no launch
            starts, dist, ops = align_editl(P, text, k, np.zeros(0, dtype=np.uint64), ops=ops_wanted)
            assert len(starts) == 0 and len(dist) == 0 and (ops.shape == (0, WORDS) if ops_wanted else ops is None)
        starts, dist, ops = align_editl_classes(byte_classes(P), text, k, [])
        assert len(starts) == 0 and len(dist) == 0 and ops.shape == (0, WORDS)


def test_a_list_longer_than_one_piece():
    """With ops a piece of the device's buffer holds (8 Mi entries) / 11 occurrences: that many + 77 ends (the same few
    thousand, tiled) go through two pieces and every copy equals its original's answer."""
    n, m, k = 4097, 12, 2
    T = draw_text("acgt", n, 7700)
    P = T[1000:1000 + m].copy()
    uniq = np.arange(n, dtype=np.uint64)  # occurrences and non-occurrences alike
    wstarts, wdist, wops = align_manyl(m, byte_accepts(P), T, uniq, k)
    assert (wdist != NONE_DIST).any() and (wdist == NONE_DIST).any()
    count = PIECE_WITH_OPS + 77
    idx = (np.arange(count, dtype=np.int64) * 2654435761) % n
    with uploaded(T) as text:
        starts, dist, ops = align_editl(P, text, k, uniq[idx])
    assert np.array_equal(starts, wstarts[idx]) and np.array_equal(dist, wdist[idx]) and np.array_equal(ops, wops[idx])


# ---- 7. refusals with a real text ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["", "_classes"])
def test_refusals_with_a_real_text(kind):
    T = draw_text("rand128", 2000, 7800)
    m = 100
    P = T[10:10 + m].copy()
    pat = byte_classes(P) if kind else P
    L = smart_amd.lib()
    f = getattr(L, "smartgpu_align_editl%s64" % kind)
    call = align_editl_classes if kind else align_editl
    with uploaded(T) as text:
        for off, n, bad in ((100, 400, 99), (100, 400, 500), (0, 2000, 2000), (0, 2000, 2**63)):
            ends = np.array([150, 160, bad, 170], dtype=np.uint64)
            starts = np.full(4, 77, dtype=np.uint64)
            dist = np.full(4, 7, dtype=np.uint8)
            ops = np.full(4 * WORDS, 5, dtype=np.uint64)
            rc = f(pat.ctypes.data, m, 9, text._h, off, n, ends.ctypes.data, 4, starts.ctypes.data, dist.ctypes.data, ops.ctypes.data)
            msg = L.smartgpu_last_error().decode()
            assert rc == -3 and "ends[2] = %d" % bad in msg and ("align_editl%s64:" % kind) in msg, (rc, msg)
            assert (starts == 77).all() and (dist == 7).all() and (ops == 5).all()  # nothing written
            with pytest.raises(SmartGpuError) as e:
                call(pat, text, 9, ends, off=off, n=n)
            assert "rc=-3" in str(e.value) and "ends[2]" in str(e.value)
        # a range outside the text
        starts = np.full(1, 77, dtype=np.uint64)
        ends = np.array([1995], dtype=np.uint64)
        assert f(pat.ctypes.data, m, 9, text._h, 1990, 11, ends.ctypes.data, 1, starts.ctypes.data, None, None) == -3 and starts[0] == 77
        assert "outside the text" in L.smartgpu_last_error().decode()
        # the bounds, with a real text: m = 257 and k = 32 name the limits
        assert f(pat.ctypes.data, 257, 9, text._h, 0, 2000, ends.ctypes.data, 1, starts.ctypes.data, None, None) == -3 and starts[0] == 77
        assert "outside [1,256]" in L.smartgpu_last_error().decode()
        assert f(pat.ctypes.data, m, 32, text._h, 0, 2000, ends.ctypes.data, 1, starts.ctypes.data, None, None) == -3 and starts[0] == 77
        assert "at most 31" in L.smartgpu_last_error().decode()
        # count == 0 with a valid text: SMARTGPU_OK, NULL lists
        assert f(pat.ctypes.data, m, 9, text._h, 0, 2000, None, 0, None, None, None) == 0
        # distances NULL, ops given: legal
        ends = np.array([10 + m - 1], dtype=np.uint64)
        starts = np.zeros(1, dtype=np.uint64)
        ops = np.zeros(WORDS, dtype=np.uint64)
        assert f(pat.ctypes.data, m, 9, text._h, 0, 2000, ends.ctypes.data, 1, starts.ctypes.data, None, ops.ctypes.data) == 0
        assert starts[0] == 10 and edit_cigar(ops) == "%d=" % m
        # more than cap occurrences: the find's refusal
        with pytest.raises(SmartGpuError, match="occurrences"):
            (find_editl_classes_align if kind else find_editl_align)(pat[:4], text, 3, cap=5)


# ---- 8. the coalescing queue -----------------------------------------------------------------------------------------------------------

def test_a_call_behind_queued_horspool_launches():
    """Plan.launch calls wait in the coalescing queue; an align call on the same text sends them first (device_ctx_flushed) and
    never enters the queue itself.  Both give their right answers."""
    from test_coalesce_gpu import cut
    rng = np.random.default_rng(7900)
    n = 3 * 32768 + 99
    T = rng.integers(0, 128, n).astype(np.uint8)
    pats = [cut(T, 1000 + 9000 * j, 16) for j in range(4)]
    for j, P in enumerate(pats):
        T[50000 + 100 * j:50000 + 100 * j + 16] = P
    Q = T[20000:20150].copy()
    T[70000:70149] = np.delete(Q, 90)
    raw = T.tobytes()

    def occurrences(P):
        c, at = 0, raw.find(P.tobytes())
        while at >= 0:
            c, at = c + 1, raw.find(P.tobytes(), at + 1)
        return c
    ends = np.array([20149, 70148, 70147, 30000], dtype=np.uint64)
    want = align_manyl(150, byte_accepts(Q), T, ends, 10)
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
                got = align_editl(Q, text, 10, ends)  # the queue is sent here
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


# ---- 9. a seeded differential fuzz -----------------------------------------------------------------------------------------------------

FUZZ_CASES, FUZZ_PARTS = 200, 4


def fuzz_case(rng):
    """(T, pat, accepts, classes?, k, off, n, ops?): a text of at most 3000 bytes over 1, 2, 4, 20 or 256 values, a range that
    begins and ends anywhere, a pattern of 1 .. 256 bytes cut from the range with up to k + 1 edits, as bytes or as classes
    with extra members, an empty or a full row now and then."""
    vals = [(97,), (0, 255), (65, 67, 71, 84), tuple(b"ACDEFGHIKLMNPQRSTVWY"), tuple(range(256))][int(rng.integers(0, 5))]
    total = int(rng.integers(1, 3001))
    T = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), total)]
    off = int(rng.integers(0, total))
    n = int(rng.integers(1, total - off + 1))
    m = int(rng.choice([1, 2, 20, 31, 32, 33, 64, 65, 100, 128, 129, 150, 200, 255, 256, int(rng.integers(1, 257))]))
    k = int(rng.choice([0, 1, 3, 7, 8, 15, 16, 31, int(rng.integers(0, 32))]))
    a = off + int(rng.integers(0, n))
    W = [int(x) for x in np.resize(T[a:a + m], m)]
    for _ in range(int(rng.integers(0, k + 2))):
        j = int(rng.integers(0, len(W)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            W[j] = int(vals[int(rng.integers(0, len(vals)))])
        elif kind == 1 and len(W) > 1:
            del W[j]
        elif len(W) < 256:
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
    """200 cases in four parts.  The ends are a random mix of the find's and arbitrary ones of the range, shuffled; the seed of
    a failing case is in every assertion message."""
    per = FUZZ_CASES // FUZZ_PARTS
    hits = misses = 0
    for case in range(part * per, (part + 1) * per):
        seed = 80000 + case
        rng = np.random.default_rng(seed)
        T, pat, accepts, classes, k, off, n, ops = fuzz_case(rng)
        find = find_editl_classes if classes else find_editl
        call = align_editl_classes if classes else align_editl
        with uploaded(T) as text:
            fends, fdist = find(pat, text, k, off=off, n=n, cap=n)
            mine = fends[rng.integers(0, len(fends), min(len(fends), 32))] if len(fends) else fends
            ends = np.concatenate([mine, (off + rng.integers(0, n, 16)).astype(np.uint64)])
            rng.shuffle(ends)
            starts, dist, words = call(pat, text, k, ends, off=off, n=n, ops=ops)
        wstarts, wdist, wwords = align_manyl(len(pat), accepts, T, ends, k, off)
        what = ("seed", seed, "classes" if classes else "bytes", len(pat), k, off, n, ops)
        assert np.array_equal(dist, wdist), (what, first_difference(dist, wdist, ends))
        assert np.array_equal(starts, wstarts), (what, first_difference(starts, wstarts, ends))
        assert (words is None) if not ops else np.array_equal(words, wwords), what
        lookup = dict(zip(fends.tolist(), fdist.tolist()))  # the find's distances at the find's ends
        assert all(lookup.get(e, NONE_DIST) == d for e, d in zip(ends.tolist(), dist.tolist())), what
        assert (starts[dist != NONE_DIST] >= off).all(), what
        hits += int((dist != NONE_DIST).sum())
        misses += int((dist == NONE_DIST).sum())
    assert hits > per and misses > per  # (the inputs: both kinds of end in number)
