"""Starts and alignments of LONG edit-distance occurrences on packed texts on the GPU (smartgpu_palign_editl64 and its sets
form; planes_editl_align of k_palignl.hip: m <= 256, k <= 31, ten words of operations per entry): starts, distances and
operations against the DEFINITION — the ten-word vector oracle of tests/test_text_alignl.py (align_manyl), every returned row
replayed — and against two independent kernels on the same bytes: text_editl_align (the bytes uploaded as a Text, bit for
bit) and, for m <= 64 and k <= 7, planes_edit_align.  Both forms of every call are checked, with ops and without.  Every
comparison is exact equality.  The kernel's unit of work is one occurrence, so texts of a few thousand symbols reach every
path; ends beyond 2^32 are in tests/test_packed_alignl_at_size_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (PackedText, Plan, SmartGpuError, align_editl, edit_cigar, engine, palign_edit, palign_editl, palign_sets_editl,  # noqa: E402
                       pfind_editl, pfind_editl_align, pfind_sets_editl, pfind_sets_editl_align)

from test_packed_align import DEL, EQ, INS, NONE_DIST, NONE_START, SUB, replay, unpack_ops  # noqa: E402
from test_packed_edit import byte_accepts, set_accepts  # noqa: E402
from test_text_alignl import WORDS, align_manyl, unpack_opsl  # noqa: E402
from test_text_edit_gpu import uploaded  # noqa: E402

ACGT = (65, 67, 71, 84)
VALUE_SETS = [(7,), (0, 255), (65, 67, 84), ACGT]  # one plane: one and two values; two planes: three and four
MS = [1, 31, 32, 33, 64, 65, 100, 128, 129, 200, 255, 256]
KS = [0, 3, 7, 8, 15, 31]
PIECE_WITH_OPS = (8 << 20) // (1 + WORDS)  # occurrences of one piece of the device's find buffer (host_ctx.hpp: kFindKeep)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def random_text(vals, n, seed):
    return np.asarray(vals, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(vals), n)]


def other(vals, v):
    return next((x for x in vals if x != v), v)


def mixed_edits(P, d, rng, vals):
    """P with d edits of the three kinds in turn at distinct places, kept apart where the pattern has the room."""
    W = [int(x) for x in P]
    if d == 0 or len(W) < 3:
        return np.asarray(W, dtype=np.uint8)
    places = sorted(rng.choice(np.arange(1, len(W) - 1), size=min(d, len(W) - 2), replace=False).tolist(), reverse=True)
    for t, j in enumerate(places):
        if t % 3 == 0:
            W[j] = other(vals, W[j])
        elif t % 3 == 1:
            del W[j]
        else:
            W.insert(j, int(vals[int(rng.integers(0, len(vals)))]))
    return np.asarray(W, dtype=np.uint8)


def first_difference(a, b, ends):
    at = int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])
    return at, int(ends[at]), int(a[at]), int(b[at])


def check(pat, accepts, T, pt, k, ends, off=0, n=None, what=None, sets=False):
    """Both forms of the call (with and without ops) against the oracle, and every hit replayed; returns (starts, distances, ops)."""
    call = palign_sets_editl if sets else palign_editl
    ends = np.asarray(ends, dtype=np.uint64)
    m = len(pat)
    wstarts, wdist, wops = align_manyl(m, accepts, T, ends, k, off)
    starts, dist, ops = call(pat, pt, k, ends, off=off, n=n)
    assert starts.dtype == np.uint64 and dist.dtype == np.uint8 and ops.dtype == np.uint64 and ops.shape == (len(ends), WORDS), what
    assert np.array_equal(dist, wdist), (what, k, first_difference(dist, wdist, ends))
    assert np.array_equal(starts, wstarts), (what, k, first_difference(starts, wstarts, ends))
    assert np.array_equal(ops, wops), (what, k, first_difference((ops != wops).any(axis=1), np.zeros(len(ends), dtype=bool), ends))
    s2, d2, o2 = call(pat, pt, k, ends, off=off, n=n, ops=False)
    assert o2 is None and np.array_equal(s2, wstarts) and np.array_equal(d2, wdist), (what, k, "ops=False")
    for s, e, d, row in zip(starts.tolist(), ends.tolist(), dist.tolist(), ops):
        if d == NONE_DIST:
            assert s == int(NONE_START) and not row.any(), (what, k, e)
        else:
            assert d <= min(k, 31) and off <= s <= e + 1 and replay(unpack_opsl(row), m, accepts, T, s, e) == d, (what, k, e)
    return starts, dist, ops


# ---- 1. lengths, k and values ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("vals", VALUE_SETS)
def test_lengths_k_and_values(vals, m):
    """A pattern cut from the text with three mixed edits, at every k: the ends are the find's (a seeded sample where there are
    many) and so are the distances, plus a seeded sample of arbitrary ends, plus the planted one.  k = 0 on the exact pattern:
    every start is e - m + 1 and the operations are m times '='."""
    n = 3001
    T = random_text(vals, n, 9000 + m)
    rng = np.random.default_rng(9100 + m)
    exact = T[1500:1500 + m].copy()
    P = mixed_edits(exact, 3, rng, vals)
    hits = misses = 0
    with PackedText.upload(T) as pt:
        assert pt.planes == (2 if len(vals) > 2 else 1)
        for k in KS:
            for pat in (exact, P) if k in (0, 31) else (P,):
                fends, fdist, cnt = pfind_editl(pat, pt, k, cap=n)
                assert cnt == len(fends)
                pick = np.sort(rng.choice(len(fends), size=min(len(fends), 96), replace=False)) if len(fends) else np.zeros(0, dtype=np.int64)
                ends = np.concatenate([fends[pick], rng.integers(0, n, 48).astype(np.uint64), np.array([1500 + m - 1], dtype=np.uint64)])
                starts, dist, ops = check(pat, byte_accepts(pat), T, pt, k, ends, what=(vals, m))
                assert np.array_equal(dist[:len(pick)], fdist[pick]), (vals, m, k)  # the distances are the find's
                lookup = dict(zip(fends.tolist(), fdist.tolist()))
                assert all(lookup.get(e, NONE_DIST) == d for e, d in zip(ends.tolist(), dist.tolist())), (vals, m, k)
                hits += int((dist != NONE_DIST).sum())
                misses += int((dist == NONE_DIST).sum())
                if k == 0 and pat is exact:
                    at = ends.tolist().index(1500 + m - 1)
                    assert int(starts[at]) == 1500 and unpack_opsl(ops[at]) == [EQ] * m, (vals, m)
                    hit = dist == 0
                    assert np.array_equal(starts[hit], ends[hit] - np.uint64(m - 1)), (vals, m)
    assert hits > 0 and (misses > 0 or len(vals) == 1 or m == 1)  # (the inputs: both kinds of end)


# ---- 2. clipping and window phases ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(33, 0), (65, 8), (100, 15), (200, 7), (256, 31)])
@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_clipping_and_window_phases(vals, m, k):
    """A range that starts at off = 129, mid-dword: the ends off .. off + m + k + 2 (every band narrower than m + k columns,
    down to one, then the first full ones; every e % 32).  A range that starts at 0: every e < 32 * 10 + 3, whose windows reach
    below dword 0 of the planes.  The last symbol of the text, whose length is no multiple of 32.  A copy of the pattern one
    symbol after off, and one that off cuts.  No start lies below off."""
    n = 2049
    T = random_text(vals, n, 9200 + m)
    P = T[1200:1200 + m].copy()
    for off, at in ((129, 130), (129, 128), (0, 1), (0, 0)):
        T2 = T.copy()
        T2[at:at + m] = P
        T2[n - m:] = P  # an occurrence that ends with the text's last symbol
        ends = set(range(off, min(off + m + k + 3, n))) | {n - 1}
        if off == 0:
            ends |= set(range(0, 32 * 10 + 3))
        ends = np.array(sorted(ends), dtype=np.uint64)
        with PackedText.upload(T2) as pt:
            starts, dist, _ = check(P, byte_accepts(P), T2, pt, k, ends, off=off, n=n - off, what=(vals, m, k, off, at))
        hit = dist != NONE_DIST
        assert (starts[hit] >= off).all() and (starts[~hit] == NONE_START).all()
        assert (int(starts[-1]), int(dist[-1])) == (n - m, 0)
        x = ends.tolist().index(at + m - 1)
        if at >= off:
            assert (int(starts[x]), int(dist[x])) == (at, 0)
        elif k >= 1:
            assert int(dist[x]) <= 1 and int(starts[x]) >= off


# ---- 3. planted edits ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_one_planted_edit_of_each_kind_at_every_pattern_position(vals):
    """m = 100, k = 2: one substitution, one deletion and one insertion at every pattern position, all in ONE text.  Compared
    against the oracle, not the planted offset, and every operation sequence replays (check).  All four operations occur."""
    m, k = 100, 2
    P = random_text(vals, m, 9300)
    gap = m + 12
    n = 3 * m * gap + 67
    T = random_text(vals, n, 9301)
    ends, a = [], 8
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
    with PackedText.upload(T) as pt:
        starts, dist, ops = check(P, byte_accepts(P), T, pt, k, ends, what=(vals, m))
    assert (dist <= 1).all()
    kinds = set()
    for row in ops:
        kinds |= set(unpack_opsl(row))
    assert kinds == {EQ, SUB, INS, DEL}


def test_a_planted_copy_with_exactly_31_mixed_edits_at_m_256():
    """31 edits of the three kinds in turn, eight symbols apart, in a copy of a 256-symbol pattern on four values: the oracle
    says D(e) = 31 for this seed (asserted), the largest distance the call reports; the same copy is no occurrence at k = 30."""
    m = 256
    rng = np.random.default_rng(9400)
    T = random_text(ACGT, 2999, 9401)
    P = random_text(ACGT, m, 9402)
    W = [int(x) for x in P]
    places = list(range(4, 4 + 31 * 8, 8))[::-1]  # 31 places, eight apart
    for t, j in enumerate(places):
        if t % 3 == 0:
            W[j] = other(ACGT, W[j])
        elif t % 3 == 1:
            del W[j]
        else:
            W.insert(j, other(ACGT, W[j - 1]))
    W = np.asarray(W, dtype=np.uint8)
    T[1500:1500 + len(W)] = W
    e = 1500 + len(W) - 1
    ends = np.arange(e - 40, e + 41, dtype=np.uint64)
    x = 40
    want = align_manyl(m, byte_accepts(P), T, ends[x:x + 1], 31)
    assert (int(want[0][0]), int(want[1][0])) == (1500, 31)  # (the input: the planted copy is 31 edits away and no fewer)
    with PackedText.upload(T) as pt:
        starts, dist, ops = check(P, byte_accepts(P), T, pt, 31, ends, what="31 edits")
        assert (int(starts[x]), int(dist[x])) == (1500, 31)
        seq = unpack_opsl(ops[x])
        assert len(seq) == int(ops[x][WORDS - 1]) and sum(seq.count(o) for o in (SUB, INS, DEL)) == 31
        fends, fdist, _ = pfind_editl(P, pt, 31, cap=len(T))
        assert e in fends.tolist() and int(fdist[fends.tolist().index(e)]) == 31
        s30, d30, o30 = check(P, byte_accepts(P), T, pt, 30, ends[x:x + 1], what="30 edits")
        assert d30[0] == NONE_DIST and not o30.any()
        rng.shuffle(ends)  # and the same ends in another order
        check(P, byte_accepts(P), T, pt, 31, ends, what="31 edits, shuffled")


# ---- 5. two differentials on the same bytes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vals", VALUE_SETS)
def test_the_byte_text_call_gives_the_same_answers_bit_for_bit(vals):
    """text_editl_align (smartgpu_align_editl64) on the same bytes uploaded as a Text is an independent kernel under the same
    contract, the fixed choice among optimal alignments included: the same starts, distances and ten words."""
    n = 2999
    T = random_text(vals, n, 9500 + len(vals))
    rng = np.random.default_rng(9501)
    with PackedText.upload(T) as pt, uploaded(T) as text:
        for m, k in ((1, 1), (33, 0), (64, 7), (65, 8), (100, 15), (150, 31), (256, 31), (256, 3)):
            P = mixed_edits(T[1300:1300 + m], min(k, 5), rng, vals)
            for off, ln in ((0, n), (129, 2500)):
                fends, _, cnt = pfind_editl(P, pt, k, off=off, n=ln, cap=n)
                assert cnt >= 1
                ends = np.concatenate([fends[rng.integers(0, cnt, min(cnt, 200))], (off + rng.integers(0, ln, 100)).astype(np.uint64)])
                a = palign_editl(P, pt, k, ends, off=off, n=ln)
                b = align_editl(P, text, k, ends, off=off, n=ln)
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (vals, m, k, off)
                a2, b2 = palign_editl(P, pt, k, ends, off=off, n=ln, ops=False), align_editl(P, text, k, ends, off=off, n=ln, ops=False)
                assert a2[2] is None and np.array_equal(a2[0], b2[0]) and np.array_equal(a2[1], b2[1]), (vals, m, k, off)


@pytest.mark.parametrize("vals", VALUE_SETS)
def test_the_short_call_gives_the_same_answers(vals):
    """For m <= 64, k <= 7 planes_edit_align (smartgpu_palign_edit64) is an independent kernel: the same starts and distances
    on the same ends, and the same operations once both packings are unpacked."""
    n = 2999
    T = random_text(vals, n, 9600 + len(vals))
    rng = np.random.default_rng(9601)
    with PackedText.upload(T) as pt:
        for m, k in ((1, 1), (12, 1), (20, 3), (32, 7), (33, 0), (64, 7)):
            P = mixed_edits(T[1300:1300 + m], min(k, 2), rng, vals)
            for off, ln in ((0, n), (129, 2500)):
                fends, _, cnt = pfind_editl(P, pt, k, off=off, n=ln, cap=n)
                assert cnt >= 1
                ends = np.concatenate([fends[:500], (off + rng.integers(0, ln, 300)).astype(np.uint64)])
                a = palign_editl(P, pt, k, ends, off=off, n=ln)
                b = palign_edit(P, pt, k, ends, off=off, n=ln)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (vals, m, k, off)
                assert all(unpack_opsl(x) == unpack_ops(y) for x, y in zip(a[2], b[2])), (vals, m, k, off)


# ---- 6. set patterns -----------------------------------------------------------------------------------------------------------------

def iupac_motif(rng, m):
    """(motif, an instance of it): letters of ACGT with N, two-member codes and full-set positions mixed in"""
    letters = np.array(list("ACGT"))[rng.integers(0, 4, m)]
    inst = letters.copy()
    two = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC"}
    for j in rng.choice(m, size=m // 4, replace=False).tolist():
        code = "N" if j % 3 == 0 else list(two)[int(rng.integers(0, 6))]
        letters[j] = code
        inst[j] = "ACGT"[int(rng.integers(0, 4))] if code == "N" else two[code][int(rng.integers(0, 2))]
    return "".join(letters.tolist()), np.frombuffer("".join(inst.tolist()).encode(), dtype=np.uint8)


def test_set_patterns():
    """An IUPAC motif of 120 symbols with N (the full set), two-member sets and — by hand — an empty set, against the oracle
    with the sets' accepts; singleton sets equal the byte-pattern call; the round trip pfind_sets_editl_align."""
    n, m = 2999, 120
    rng = np.random.default_rng(9700)
    motif, inst = iupac_motif(rng, m)
    assert "N" in motif and any(c in motif for c in "RYSWKM")
    T = random_text(ACGT, n, 9701)
    T[300:300 + m] = inst
    T[1000:1000 + m - 1] = np.delete(inst, 50)
    T[2000:2000 + m + 1] = np.insert(inst, 30, other(ACGT, inst[29]))
    with PackedText.upload(T) as pt:
        sets = pt.iupac(motif)
        sets[70] = 0  # an empty set: it accepts nothing, every alignment pays for it
        assert (sets == 15).any() and (sets == 0).sum() == 1 and any(bin(int(s)).count("1") == 2 for s in sets)
        accepts = set_accepts(sets, ACGT)
        for k in (3, 12):
            ends, fdist, cnt = pfind_sets_editl(sets, pt, k, cap=n)
            assert cnt >= 3 and {300 + m - 1, 1000 + m - 2, 2000 + m} <= set(ends.tolist()) and fdist.min() >= 1
            ends = np.concatenate([ends, rng.integers(0, n, 64).astype(np.uint64)])
            starts, dist, ops = check(sets, accepts, T, pt, k, ends, what=("iupac", k), sets=True)
            assert np.array_equal(dist[:cnt], fdist)
        starts, ends, dist, ops, cnt = pfind_sets_editl_align(sets, pt, 3, cap=n)
        w = align_manyl(m, accepts, T, ends, 3)
        assert cnt == len(ends) >= 3 and np.array_equal(starts, w[0]) and np.array_equal(dist, w[1]) and np.array_equal(ops, w[2])
        P = T[1500:1500 + 150].copy()
        P[20] = other(ACGT, P[20])
        single = np.array([1 << ACGT.index(b) for b in P.tolist()], dtype=np.uint8)
        ends, _, cnt = pfind_editl(P, pt, 3, cap=n)
        assert cnt >= 1
        a, b = palign_editl(P, pt, 3, ends), palign_sets_editl(single, pt, 3, ends)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_refusals_with_a_real_text():
    """A set naming a code the text does not hold (the position is in the message), a three-plane text (the other edit calls'
    message), an end outside the range (by index and value), a range outside the text, the bounds; nothing is written."""
    T = random_text((65, 67, 84), 2049, 9800)
    m = 100
    P = T[10:10 + m].copy()
    L = smart_amd.lib()
    with PackedText.upload(T) as pt:
        sets = np.full(m, 1, dtype=np.uint8)
        sets[57] = 8  # code 3 on a text of three values
        with pytest.raises(SmartGpuError) as e:
            palign_sets_editl(sets, pt, 9, np.array([500], dtype=np.uint64))
        assert "position 57" in str(e.value) and "names a code >= 3" in str(e.value)
        for kind, pat in (("", P), ("_sets", np.full(m, 1, dtype=np.uint8))):
            f = getattr(L, "smartgpu_palign%s_editl64" % kind)
            call = palign_sets_editl if kind else palign_editl
            for off, n, bad in ((100, 400, 99), (100, 400, 500), (0, 2049, 2049), (0, 2049, 2**63)):
                ends = np.array([150, 160, bad, 170], dtype=np.uint64)
                starts = np.full(4, 77, dtype=np.uint64)
                dist = np.full(4, 7, dtype=np.uint8)
                ops = np.full(4 * WORDS, 5, dtype=np.uint64)
                rc = f(pat.ctypes.data, m, 9, pt._h, off, n, ends.ctypes.data, 4, starts.ctypes.data, dist.ctypes.data, ops.ctypes.data)
                msg = L.smartgpu_last_error().decode()
                assert rc == -3 and "ends[2] = %d" % bad in msg and ("palign%s_editl64:" % kind) in msg, (rc, msg)
                assert (starts == 77).all() and (dist == 7).all() and (ops == 5).all()  # nothing written
                with pytest.raises(SmartGpuError) as e:
                    call(pat, pt, 9, ends, off=off, n=n)
                assert "rc=-3" in str(e.value) and "ends[2]" in str(e.value)
            starts = np.full(1, 77, dtype=np.uint64)
            ends = np.array([2045], dtype=np.uint64)
            assert f(pat.ctypes.data, m, 9, pt._h, 2040, 10, ends.ctypes.data, 1, starts.ctypes.data, None, None) == -3 and starts[0] == 77
            assert "outside the packed text" in L.smartgpu_last_error().decode()
            assert f(pat.ctypes.data, 257, 9, pt._h, 0, 2049, ends.ctypes.data, 1, starts.ctypes.data, None, None) == -3 and starts[0] == 77
            assert "outside [1,256]" in L.smartgpu_last_error().decode()
            assert f(pat.ctypes.data, m, 32, pt._h, 0, 2049, ends.ctypes.data, 1, starts.ctypes.data, None, None) == -3 and starts[0] == 77
            assert "at most 31" in L.smartgpu_last_error().decode()
            assert f(pat.ctypes.data, m, 9, pt._h, 0, 2049, None, 0, None, None, None) == 0  # count == 0: SMARTGPU_OK, NULL lists
        # distances NULL, ops given: legal
        ends = np.array([10 + m - 1], dtype=np.uint64)
        starts = np.zeros(1, dtype=np.uint64)
        ops = np.zeros(WORDS, dtype=np.uint64)
        assert L.smartgpu_palign_editl64(P.ctypes.data, m, 9, pt._h, 0, 2049, ends.ctypes.data, 1, starts.ctypes.data, None, ops.ctypes.data) == 0
        assert starts[0] == 10 and edit_cigar(ops) == "%d=" % m
    T5 = random_text((45, 65, 67, 71, 84), 2049, 9801)
    with PackedText.upload(T5, wide=True) as pt3:
        assert pt3.planes == 3
        for call, pat in ((palign_editl, T5[10:110].copy()), (palign_sets_editl, np.full(100, 1, dtype=np.uint8))):
            with pytest.raises(SmartGpuError, match="three-plane texts .* are not offered here: edit distance and alignments read one or two planes"):
                call(pat, pt3, 3, np.array([500], dtype=np.uint64))


# ---- 7. the list's shape -----------------------------------------------------------------------------------------------------------

def test_the_shape_of_the_list():
    """Duplicates, descending order, count = 1 and count = 0 — and counts around the four waves of a workgroup — from one text:
    entry for entry what the sorted unique run gives, with ops and without."""
    m, k, n = 100, 3, 3001
    rng = np.random.default_rng(9900)
    P = random_text(ACGT, m, 9901)
    T = random_text(ACGT, n, 9902)
    for t, a in enumerate(range(20, n - 2 * m, 130)):  # a copy with 0 .. 3 mixed edits every 130 symbols
        W = mixed_edits(P, t % 4, rng, ACGT)
        T[a:a + len(W)] = W
    with PackedText.upload(T) as pt:
        all_ends, _, cnt = pfind_editl(P, pt, k, cap=n)
        assert cnt >= 15
        all_ends = np.concatenate([all_ends[:120], np.arange(1000, 1040, dtype=np.uint64)])
        s0, d0, o0 = check(P, byte_accepts(P), T, pt, k, all_ends, what="sorted")
        assert (d0 != NONE_DIST).any() and (d0 == NONE_DIST).any()
        base = {e: (int(s0[x]), int(d0[x]), o0[x].tolist()) for x, e in enumerate(all_ends.tolist())}
        for count in (1, 3, 4, 5, 257, 5000):
            ends = all_ends[rng.integers(0, len(all_ends), count)]  # shuffled, duplicates included
            if count >= 257:
                assert len(np.unique(ends)) < count
            for order in (ends, np.sort(ends)[::-1].copy()):  # as drawn, and descending
                starts, dist, ops = palign_editl(P, pt, k, order)
                for x, e in enumerate(order.tolist()):
                    assert (int(starts[x]), int(dist[x]), ops[x].tolist()) == base[e], (count, x, e)
                s2, d2, o2 = palign_editl(P, pt, k, order, ops=False)
                assert o2 is None and np.array_equal(s2, starts) and np.array_equal(d2, dist)
        for ops_wanted in (True, False):  # count == 0: empty arrays, no launch
            starts, dist, ops = palign_editl(P, pt, k, np.zeros(0, dtype=np.uint64), ops=ops_wanted)
            assert len(starts) == 0 and len(dist) == 0 and (ops.shape == (0, WORDS) if ops_wanted else ops is None)
        starts, dist, ops = palign_sets_editl(np.full(m, 15, dtype=np.uint8), pt, k, [])
        assert len(starts) == 0 and len(dist) == 0 and ops.shape == (0, WORDS)


def test_a_list_one_longer_than_a_piece():
    """With ops a piece of the device's buffer holds (8 Mi entries) / 11 occurrences: that many + 1 ends (the same few
    thousand, tiled) at m = 65 go through two pieces and every copy equals its original's answer."""
    n, m, k = 2049, 65, 4
    T = random_text(ACGT, n, 9950)
    P = mixed_edits(T[1000:1000 + m + 1], 2, np.random.default_rng(9951), ACGT)  # one substitution, one symbol removed
    assert len(P) == m
    uniq = np.arange(n, dtype=np.uint64)  # occurrences and non-occurrences alike
    wstarts, wdist, wops = align_manyl(m, byte_accepts(P), T, uniq, k)
    assert (wdist != NONE_DIST).any() and (wdist == NONE_DIST).any()
    count = PIECE_WITH_OPS + 1
    idx = (np.arange(count, dtype=np.int64) * 2654435761) % n
    with PackedText.upload(T) as pt:
        starts, dist, ops = palign_editl(P, pt, k, uniq[idx])
    assert np.array_equal(starts, wstarts[idx]) and np.array_equal(dist, wdist[idx]) and np.array_equal(ops, wops[idx])


# ---- 8. ordering ---------------------------------------------------------------------------------------------------------------------

def test_a_call_behind_queued_horspool_launches():
    """Plan.launch calls wait in the coalescing queue; an align call on the same device sends them first (device_ctx_flushed)
    and never enters the queue itself.  Both give their right answers."""
    from test_coalesce_gpu import cut
    rng = np.random.default_rng(9960)
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
    D = random_text(ACGT, 3001, 9961)
    Q = D[1000:1150].copy()
    D[2000:2149] = np.delete(Q, 90)
    ends = np.array([1149, 2148, 2147, 500], dtype=np.uint64)
    want = align_manyl(150, byte_accepts(Q), D, ends, 10)
    assert want[1].tolist()[:2] == [0, 1] and want[1][3] == NONE_DIST
    default = engine.coalesce(8)
    try:
        with uploaded(T) as text, PackedText.upload(D) as pt:
            plans = [Plan("hor", P) for P in pats]
            try:
                engine.device_sync(0)
                l0, p0 = engine.coalesce_stats(0)
                for pl in plans:
                    pl.launch(text)
                got = palign_editl(Q, pt, 10, ends)  # the queue is sent here
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


def test_find_then_align_round_trip():
    """pfind_editl_align: the find's ends and distances, the align call's starts and operations, equal to the oracle's; more
    than cap occurrences give the count alone."""
    n, m, k = 3001, 150, 9
    rng = np.random.default_rng(9970)
    T = random_text(ACGT, n, 9971)
    P = random_text(ACGT, m, 9972)
    for t, a in enumerate(range(40, n - 2 * m, 333)):
        W = mixed_edits(P, t % 7, rng, ACGT)
        T[a:a + len(W)] = W
    with PackedText.upload(T) as pt:
        starts, ends, dist, ops, cnt = pfind_editl_align(P, pt, k, cap=n)
        fends, fdist, fcnt = pfind_editl(P, pt, k, cap=n)
        assert cnt == fcnt == len(ends) >= 8 and np.array_equal(ends, fends) and np.array_equal(dist, fdist)
        w = align_manyl(m, byte_accepts(P), T, ends, k)
        assert np.array_equal(starts, w[0]) and np.array_equal(dist, w[1]) and np.array_equal(ops, w[2])
        assert all(replay(unpack_opsl(r), m, byte_accepts(P), T, s, e) == d for s, e, d, r in zip(starts.tolist(), ends.tolist(), dist.tolist(), ops))
        assert pfind_editl_align(P, pt, k, cap=3) == (None, None, None, None, cnt)


# ---- 9. a seeded differential fuzz -----------------------------------------------------------------------------------------------------

FUZZ_CASES, FUZZ_PARTS = 240, 4


def fuzz_text(rng, vals, total):
    """uniform, skewed (one value in 16 is another), or run-heavy (runs of 1 .. 40 equal symbols)"""
    kind = int(rng.integers(0, 3))
    if kind == 0 or len(vals) == 1:
        return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), total)]
    if kind == 1:
        rare = rng.integers(0, 16, total) == 0
        return np.where(rare, np.asarray(vals, dtype=np.uint8)[rng.integers(1, len(vals), total)], np.uint8(vals[0])).astype(np.uint8)
    runs = np.repeat(np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), total)], rng.integers(1, 41, total))
    return runs[:total].copy()


def fuzz_case(rng, k):
    """(T, pat, accepts, sets?, off, n, ops?): a text of at most 3000 symbols over 1 .. 4 values, a range that begins and ends
    anywhere (mid-dword as a rule), a pattern of 1 .. 256 symbols cut from the range with up to k + 1 edits, as bytes or as sets
    with extra members, an empty or a full set now and then."""
    vals = VALUE_SETS[int(rng.integers(0, 4))]
    total = int(rng.integers(1, 3001))
    T = fuzz_text(rng, vals, total)
    off = int(rng.integers(0, total))
    n = int(rng.integers(1, total - off + 1))
    m = int(rng.choice([1, 2, 20, 31, 32, 33, 64, 65, 100, 128, 129, 150, 200, 255, 256, int(rng.integers(1, 257))]))
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
    present = tuple(np.unique(T).tolist())  # the codes are ranks among the values the TEXT holds
    if rng.integers(0, 2) == 0:
        return T, P, byte_accepts(P), False, off, n, bool(rng.integers(0, 2))
    sets = np.array([1 << present.index(b) if b in present else 0 for b in P.tolist()], dtype=np.uint8)
    for j in range(len(P)):
        for _ in range(int(rng.integers(0, 3)) // 2):
            sets[j] |= 1 << int(rng.integers(0, len(present)))
    if rng.integers(0, 4) == 0:
        sets[int(rng.integers(0, len(P)))] = 0
    if rng.integers(0, 4) == 0:
        sets[int(rng.integers(0, len(P)))] = (1 << len(present)) - 1
    return T, sets, set_accepts(sets, present), True, off, n, bool(rng.integers(0, 2))


@pytest.mark.parametrize("part", range(FUZZ_PARTS))
def test_seeded_differential_fuzz(part):
    """240 cases in four parts; case c runs at k = c % 32, so every k is covered.  The ends are a random mix of the find's and
    arbitrary ones of the range, shuffled; compared with the oracle and — the plain form — with align_editl on the same bytes.
    The seed of a failing case is in every assertion message."""
    per = FUZZ_CASES // FUZZ_PARTS
    hits = misses = 0
    for case in range(part * per, (part + 1) * per):
        seed, k = 90000 + case, case % 32
        rng = np.random.default_rng(seed)
        T, pat, accepts, sets, off, n, ops = fuzz_case(rng, k)
        find = pfind_sets_editl if sets else pfind_editl
        call = palign_sets_editl if sets else palign_editl
        what = ("seed", seed, "sets" if sets else "bytes", len(pat), k, off, n, ops)
        with PackedText.upload(T) as pt:
            fends, fdist, cnt = find(pat, pt, k, off=off, n=n, cap=n)
            mine = fends[rng.integers(0, len(fends), min(len(fends), 32))] if len(fends) else fends
            ends = np.concatenate([mine, (off + rng.integers(0, n, 16)).astype(np.uint64)])
            rng.shuffle(ends)
            starts, dist, words = call(pat, pt, k, ends, off=off, n=n, ops=ops)
            if not sets:
                with uploaded(T) as text:
                    b = align_editl(pat, text, k, ends, off=off, n=n, ops=ops)
                assert np.array_equal(starts, b[0]) and np.array_equal(dist, b[1]) and ((words is None and b[2] is None) or np.array_equal(words, b[2])), what
        wstarts, wdist, wwords = align_manyl(len(pat), accepts, T, ends, k, off)
        assert np.array_equal(dist, wdist), (what, first_difference(dist, wdist, ends))
        assert np.array_equal(starts, wstarts), (what, first_difference(starts, wstarts, ends))
        assert (words is None) if not ops else np.array_equal(words, wwords), what
        lookup = dict(zip(fends.tolist(), fdist.tolist()))  # the find's distances at the find's ends
        assert all(lookup.get(e, NONE_DIST) == d for e, d in zip(ends.tolist(), dist.tolist())), what
        assert (starts[dist != NONE_DIST] >= off).all(), what
        hits += int((dist != NONE_DIST).sum())
        misses += int((dist == NONE_DIST).sum())
    assert hits > per and misses > per  # (the inputs: both kinds of end in number)
