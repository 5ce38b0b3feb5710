"""Packed texts of five to eight values on three bit planes on the GPU (planes3_pack, planes3_scan, planes3_find): the pack,
and the counts, positions and distances of the ten calls against the DEFINITION, computed here with numpy over codes — the
distance of start position s is the number of j < m for which the code of T[s + j] is not a member of sets[j] (a byte pattern:
the singleton of its byte's code, the empty set for a byte the text does not hold), and s is an occurrence when it is at most
k.  Every comparison is exact equality; no text is longer than 2^20 + 3 symbols."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (PackedText, Text, engine, pfind, pfind_batch, pfind_mis, pfind_sets, pfind_sets_mis, psearch, psearch_batch,  # noqa: E402
                       psearch_mis, psearch_sets, psearch_sets_mis)

ACGNT = (65, 67, 71, 78, 84)
EIGHT = (0, 1, 2, 3, 4, 5, 6, 255)
SIX = (10, 45, 65, 67, 71, 84)
VALUE_SETS = [ACGNT, EIGHT, SIX]
NS = [33, 4097, 2**20 + 3]
MS = [1, 2, 8, 31, 32, 33, 64, 65, 200, 4200]
ERR_ARG, ERR_NOMEM = -3, -5
BATCH_BOUND = 7884  # include/smartgpu.h: patterns per batch call on a three-plane text


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def random_text(vals, n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]


def codes_of(T, vals):
    """The code of every symbol: the rank of its byte among the text's values."""
    return np.searchsorted(np.asarray(sorted(vals), dtype=np.uint8), T).astype(np.uint8)


def sets_of(P, vals):
    """A byte pattern as sets: the singleton of each byte's code, the empty set for a byte the text does not hold."""
    P = np.asarray(P, dtype=np.uint8)
    v = np.asarray(sorted(vals), dtype=np.uint8)
    c = np.minimum(np.searchsorted(v, P), len(v) - 1)
    return np.where(v[c] == P, 1 << c, 0).astype(np.uint8)


def by_definition(sets, T, vals, k, off=0, n=None):
    """(ascending start positions relative to symbol 0 as uint64, their distances as uint8) in [off, off + n - m].  The first
    positions of the pattern are summed over all start positions at once (slices), then a progressive filter: the
    candidates' running counts of non-members, candidates dropped once they are over k."""
    sets = np.asarray(sets, dtype=np.uint8)
    n = len(T) - off if n is None else n
    m = len(sets)
    if m > n:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    code = codes_of(T, vals)
    miss = [np.array([not (int(x) >> c) & 1 for c in range(8)], dtype=np.uint8) for x in sets]  # miss[j][code]
    starts = n - m + 1
    head = min(m, 24)
    d = np.zeros(starts, dtype=np.uint8)
    for j in range(head):
        d += miss[j][code[off + j:off + j + starts]]
    keep = d <= k
    s = off + np.flatnonzero(keep).astype(np.int64)
    d = d[keep].astype(np.int32)
    for j in range(head, m):
        if len(s) == 0:
            break
        d += miss[j][code[s + j]]
        keep = d <= k
        if not keep.all():
            s, d = s[keep], d[keep]
    return s.astype(np.uint64), d.astype(np.uint8)


def check_sets(sets, T, vals, pt, k, off=0, n=None, what=None):
    """Count, positions and distances of the set calls against the definition (k = 0: the calls without k as well);
    returns (positions, distances)."""
    sets = np.asarray(sets, dtype=np.uint8)
    wpos, wdist = by_definition(sets, T, vals, k, off, n)
    got = psearch_sets_mis(sets, pt, k, off=off, n=n)[0]
    assert got == len(wpos), (what, "psearch_sets_mis", got, len(wpos))
    pos, dist, cnt = pfind_sets_mis(sets, pt, k, off=off, n=n, cap=max(len(wpos), 1))
    assert cnt == len(wpos) and pos is not None and pos.dtype == np.uint64 and dist.dtype == np.uint8, (what, cnt, len(wpos))
    assert np.array_equal(pos, wpos) and np.array_equal(dist, wdist), (what, "pfind_sets_mis")
    if k == 0:
        assert psearch_sets(sets, pt, off=off, n=n)[0] == len(wpos), (what, "psearch_sets")
        spos, scnt = pfind_sets(sets, pt, off=off, n=n, cap=max(len(wpos), 1))
        assert scnt == len(wpos) and np.array_equal(spos, wpos), (what, "pfind_sets")
    return pos, dist


def check_bytes(P, T, vals, pt, k, off=0, n=None, what=None):
    """The same for a byte pattern: the mismatch calls, and with k = 0 the exact calls."""
    P = np.asarray(P, dtype=np.uint8)
    wpos, wdist = by_definition(sets_of(P, vals), T, vals, k, off, n)
    got = psearch_mis(P, pt, k, off=off, n=n)[0]
    assert got == len(wpos), (what, "psearch_mis", got, len(wpos))
    pos, dist, cnt = pfind_mis(P, pt, k, off=off, n=n, cap=max(len(wpos), 1))
    assert cnt == len(wpos) and pos is not None and pos.dtype == np.uint64 and dist.dtype == np.uint8, (what, cnt, len(wpos))
    assert np.array_equal(pos, wpos) and np.array_equal(dist, wdist), (what, "pfind_mis")
    if k == 0:
        assert psearch(P, pt, off=off, n=n)[0] == len(wpos), (what, "psearch")
        epos, ecnt = pfind(P, pt, off=off, n=n, cap=max(len(wpos), 1))
        assert ecnt == len(wpos) and epos.dtype == np.uint64 and np.array_equal(epos, wpos), (what, "pfind")
    return pos, dist


def other_value(vals, v, rng):
    rest = [x for x in vals if x != v]
    return rest[int(rng.integers(0, len(rest)))]


def plant(T, at, P, d, vals, rng):
    """P at T[at:] with d substituted positions (distinct, seeded)."""
    W = np.array(P, dtype=np.uint8)
    for j in rng.choice(len(W), size=d, replace=False):
        W[j] = other_value(vals, W[j], rng)
    T[at:at + len(W)] = W
    return W


def iupac_like(window, vals, rng, extra=0.3):
    """Sets that accept `window`: the singleton of each of its symbols, with every other code added with probability `extra`."""
    s = sets_of(window, vals)
    for c in range(len(vals)):
        s |= ((rng.random(len(window)) < extra).astype(np.uint8) << c).astype(np.uint8)
    return s


# ---- the pack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vals", VALUE_SETS)
@pytest.mark.parametrize("n", NS)
def test_pack_round_trip(vals, n):
    T = random_text(vals, n, 100 + n + len(vals))
    T[:len(vals)] = vals  # every value occurs
    with PackedText.upload(T, wide=True) as pt:
        assert len(pt) == n and pt.planes == 3 and pt.symbols() == list(vals)
        planes, plane_bytes = smart_amd.ptext_layout8(n, len(vals))
        assert planes == 3 and pt.nbytes == 3 * plane_bytes
        assert np.array_equal(pt.read(0, n), T)
        assert np.array_equal(pt.read(n - 33, 33), T[n - 33:]) and np.array_equal(pt.read(17, 15), T[17:32])
    text = Text.upload(T)
    try:
        with PackedText.pack(text, wide=True) as pt:
            assert pt.planes == 3 and pt.symbols() == list(vals) and np.array_equal(pt.read(0, n), T)
        assert np.array_equal(text.read(0, n), T)  # the byte text stays valid
    finally:
        text.free()


def test_wide_pack_of_at_most_four_values_is_the_narrow_pack():
    for vals in [(65, 67, 71, 84), (65, 67, 84), (0, 255), (7,)]:
        T = random_text(vals, 4097, 200 + len(vals))
        T[:len(vals)] = vals
        P = T[2000:2000 + (3 if len(vals) > 1 else 5)].copy()
        with PackedText.upload(T, wide=True) as w, PackedText.upload(T) as nw:
            assert (w.planes, w.nbytes, w.symbols(), len(w)) == (nw.planes, nw.nbytes, nw.symbols(), len(nw))
            assert w.planes == (2 if len(vals) > 2 else 1)
            assert np.array_equal(w.read(0, 4097), T)
            assert psearch(P, w)[0] == psearch(P, nw)[0] > 0
            a, b = pfind(P, w), pfind(P, nw)
            assert a[1] == b[1] and np.array_equal(a[0], b[0])
            a, b = pfind_mis(P, w, 1), pfind_mis(P, nw, 1)
            assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            vals4 = np.zeros(4, dtype=np.uint8)
            assert engine.lib().smartgpu_ptext_symbols(w._h, vals4.ctypes.data) == len(vals)  # the four-entry call serves it


def test_more_than_eight_values_are_refused():
    T = np.arange(9, dtype=np.uint8).repeat(5)
    with pytest.raises(smart_amd.SmartGpuError, match="9 distinct"):
        PackedText.upload(T, wide=True)
    five = random_text(ACGNT, 100, 3)
    five[:5] = ACGNT
    with pytest.raises(smart_amd.SmartGpuError, match="5 distinct byte values: a packed text holds at most 4"):
        PackedText.upload(five)  # the four-value constructor refuses as before


def test_the_four_entry_symbols_call_is_refused_on_three_planes():
    T = random_text(ACGNT, 100, 4)
    T[:5] = ACGNT
    with PackedText.upload(T, wide=True) as pt:
        vals = np.full(4, 0xEE, dtype=np.uint8)
        assert engine.lib().smartgpu_ptext_symbols(pt._h, vals.ctypes.data) == ERR_ARG
        assert "smartgpu_ptext_symbols8" in engine.lib().smartgpu_last_error().decode()
        assert (vals == 0xEE).all()


# ---- exact count and find ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vals", VALUE_SETS)
@pytest.mark.parametrize("n", NS)
def test_exact_count_and_find(vals, n):
    rng = np.random.default_rng(300 + n + len(vals))
    T = random_text(vals, n, 310 + n + len(vals))
    T[:len(vals)] = vals
    # every pattern is cut from the text's END — an occurrence ending at the last symbol — and, where the text has the room,
    # planted once more in a stretch of its own below the longest pattern's tail
    step = 0 if n < 4097 else 450 if n == 4097 else 10000
    plan = []
    tail = n - max(m for m in MS if m <= n)
    for i, m in enumerate(MS):
        if m > n:
            continue
        assert not step or 64 + step * i + m <= tail
        P = T[n - m:].copy()
        if step:
            plant(T, 64 + step * i, P, 0, vals, rng)
        plan.append((m, P, 64 + step * i if step else None))
    with PackedText.upload(T, wide=True) as pt:
        assert pt.planes == 3 and len(plan) >= 6
        for m, P, planted in plan:
            pos, dist = check_bytes(P, T, vals, pt, 0, what=(vals, n, m))
            assert n - m in pos.tolist() and not dist.any(), (vals, n, m)
            assert planted is None or planted in pos.tolist(), (vals, n, m)
            if m < n:
                F = P.copy()
                F[m // 2] = 200  # a byte the text does not hold
                assert psearch(F, pt)[0] == 0 and pfind(F, pt)[1] == 0, (vals, n, m)


@pytest.mark.parametrize("vals", [ACGNT, EIGHT])
def test_overlapping_and_periodic_occurrences(vals):
    n = 4097
    unit = np.asarray([vals[4], vals[0], vals[4]], dtype=np.uint8)
    T = np.resize(unit, n)  # period 3: xyxxyxxyx...
    T[1000:1100] = vals[-1]  # a run: a pattern of one value overlaps itself at every position
    T[5:5 + len(vals)] = vals
    with PackedText.upload(T, wide=True) as pt:
        for m in (1, 2, 8, 33, 65, 200):
            pos, _ = check_bytes(np.resize(unit, m), T, vals, pt, 0, what=("periodic", m))
            assert len(pos) > 100
            run = np.full(min(m, 100), vals[-1], dtype=np.uint8)
            pos, _ = check_bytes(run, T, vals, pt, 0, what=("run", m))
            assert len(pos) >= 100 - len(run) + 1


@pytest.mark.parametrize("vals", VALUE_SETS)
@pytest.mark.parametrize("n", NS)
def test_the_pad_is_not_text(vals, n):
    """Pad and tail bits are zero and look like code 0: a pattern of values[0] at the text's end must stop at the end."""
    T = random_text(vals, n, 400 + n + len(vals))
    T[:len(vals)] = vals
    tail = min(n - len(vals), 70)
    T[n - tail:] = vals[0]
    with PackedText.upload(T, wide=True) as pt:
        for m in (1, 2, 8, 31, 32, 33, 64, 65):
            if m > tail:
                continue
            P = np.full(m, vals[0], dtype=np.uint8)
            pos, _ = check_bytes(P, T, vals, pt, 0, what=(vals, n, m))
            assert int(pos[-1]) == n - m
            check_bytes(P, T, vals, pt, 3, what=(vals, n, m, "k=3"))
        if n < 4200:  # m > n: no window fits, whatever the pad holds
            long = np.full(n + 1, vals[0], dtype=np.uint8)
            assert psearch(long, pt)[0] == 0 and pfind(long, pt)[1] == 0 and psearch_mis(long, pt, 7)[0] == 0


# ---- sets ----------------------------------------------------------------------------------------------------------------
def test_every_set_at_one_position():
    vals, n = EIGHT, 4097
    T = random_text(vals, n, 500)
    with PackedText.upload(T, wide=True) as pt:
        for s in range(1, 256):
            sets = np.array([1 << int(codes_of(T[77:78], vals)[0]), s, 255], dtype=np.uint8)
            pos, _ = check_sets(sets, T, vals, pt, 0, what=("set", s))
            assert len(pos) > 0
            if s in (1, 0x10, 0x81, 0x0F, 0xF0, 0x33, 0xFE):  # the step's cases, with a counter too
                check_sets(sets, T, vals, pt, 1, what=("set k=1", s))
                check_sets(np.array([s], dtype=np.uint8), T, vals, pt, 0, what=("alone", s))


@pytest.mark.parametrize("vals", [ACGNT, EIGHT])
def test_every_position_with_a_few_sets(vals):
    """Pattern positions 0 .. 39: the 32nd is where the kernel arguments end and the verification begins."""
    n, m = 4097, 40
    rng = np.random.default_rng(510 + len(vals))
    T = random_text(vals, n, 511 + len(vals))
    W = T[1000:1000 + m].copy()
    plant(T, 3000, W, 0, vals, rng)
    allv = (1 << len(vals)) - 1
    with PackedText.upload(T, wide=True) as pt:
        for j in range(m):
            own = int(sets_of(W[j:j + 1], vals)[0])
            for s in (own | 1, own | 0x10, allv & ~own, allv):
                sets = sets_of(W, vals)
                sets[j] = s
                pos, _ = check_sets(sets, T, vals, pt, 0, what=(vals, j, s))
                assert ({1000, 3000} <= set(pos.tolist())) == bool(s & own)
            sets = np.full(m, allv, dtype=np.uint8)  # every other position full: only position j decides
            sets[j] = own
            pos, _ = check_sets(sets, T, vals, pt, 0, what=(vals, j, "alone"))
            assert len(pos) > n // 16


def test_full_and_empty_sets():
    vals, n = SIX, 4097
    T = random_text(vals, n, 520)
    T[:6] = vals
    allv = 63
    with PackedText.upload(T, wide=True) as pt:
        for m in (1, 8, 33, 70):
            full = np.full(m, allv, dtype=np.uint8)
            assert psearch_sets(full, pt)[0] == n - m + 1  # every start position
            pos, cnt = pfind_sets(full, pt, cap=n)
            assert cnt == n - m + 1 and np.array_equal(pos, np.arange(n - m + 1, dtype=np.uint64))
            check_sets(full, T, vals, pt, 2, what=("full k=2", m))
            mixed = iupac_like(T[900:900 + m], vals, np.random.default_rng(m))
            mixed[::3] = allv
            check_sets(mixed, T, vals, pt, 0, what=("mixed", m))
            empty = mixed.copy()
            empty[m // 2] = 0
            assert psearch_sets(empty, pt)[0] == 0 and pfind_sets(empty, pt)[1] == 0
            check_sets(empty, T, vals, pt, 0, what=("empty k=0", m))
            pos, dist = check_sets(empty, T, vals, pt, 2, what=("empty k=2", m))  # the empty set is counted into the distance
            assert len(pos) > 0 and dist.min() >= 1


def test_an_unknown_base_of_the_text_matches_nothing():
    n = 4097
    T = random_text((65, 67, 71, 84), n, 530)
    T[17] = 78
    motif = "GANTCWGATNCAGTCA"
    inst = np.frombuffer(motif.replace("N", "C").replace("W", "A").encode(), dtype=np.uint8)
    T[1000:1016] = inst
    T[2000:2016] = inst
    T[2002] = 78  # an N inside an otherwise matching window, under the motif's own N
    T[3000:3016] = inst
    T[3000] = 78  # and under a plain letter
    with PackedText.upload(T, wide=True) as pt:
        assert pt.symbols() == list(ACGNT)
        sets = pt.iupac(motif)
        assert sets.tolist() == smart_amd.iupac_sets(motif, ACGNT, wide=True).tolist() and not (sets & 8).any()
        pos, _ = check_sets(sets, T, ACGNT, pt, 0, what="motif")
        assert 1000 in pos.tolist() and 2000 not in pos.tolist() and 3000 not in pos.tolist()
        pos, dist = check_sets(sets, T, ACGNT, pt, 1, what="motif k=1")  # with one mismatch both are found, at distance 1
        at = pos.tolist()
        assert dist[at.index(2000)] == 1 and dist[at.index(3000)] == 1 and dist[at.index(1000)] == 0


# ---- mismatches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(8))
def test_mismatch_boundaries(k):
    """Windows planted at distances k - 1, k and k + 1: the counter's boundaries (1, 3 and 7 are where it gains a bit)."""
    for vi, vals in enumerate(VALUE_SETS):
        n = 4097
        rng = np.random.default_rng(600 + 10 * k + vi)
        for m in (20, 33, 70):
            T = random_text(vals, n, 601 + 10 * k + vi + m)
            T[:len(vals)] = vals
            P = random_text(vals, m, 602 + 10 * k + vi + m)
            ats = {}
            for i, d in enumerate(x for x in (k - 1, k, k + 1) if x >= 0):
                ats[d] = 500 + 900 * i + 31 * i
                plant(T, ats[d], P, d, vals, rng)
            T[n - m:] = P  # and an exact copy at the very end
            with PackedText.upload(T, wide=True) as pt:
                pos, dist = check_bytes(P, T, vals, pt, k, what=(vals, k, m))
                at = pos.tolist()
                for d, a in ats.items():
                    assert (a in at) == (d <= k), (vals, k, m, d)
                    if d <= k:
                        assert dist[at.index(a)] == d
                sets = iupac_like(P, vals, rng, extra=0.15)
                check_sets(sets, T, vals, pt, k, what=(vals, k, m, "sets"))
                assert np.array_equal(check_sets(sets_of(P, vals), T, vals, pt, k, what="singletons")[0], pos)  # singleton sets: the mismatch answers


def test_saturation_and_k_at_least_m():
    vals, n = EIGHT, 2**16 + 5
    rng = np.random.default_rng(610)
    T = random_text(vals, n, 611)
    for m in (600, 4200):  # a random window differs in 7/8 of its positions: hundreds of mismatches wrap the counter
        P = random_text(vals, m, 612 + m)
        plant(T, 1000, P, 7, vals, rng)
        plant(T, 20000, P, 8, vals, rng)
        with PackedText.upload(T, wide=True) as pt:
            for k in (1, 3, 7):
                pos, dist = check_bytes(P, T, vals, pt, k, what=("saturation", m, k))
                assert pos.tolist() == ([1000] if k == 7 else []) and dist.tolist() == ([7] if k == 7 else [])
    with PackedText.upload(T, wide=True) as pt:
        for m, k in ((1, 1), (3, 5), (7, 7), (2, 7)):  # k >= m: every start position, its distance still reported
            P = random_text(vals, m, 620 + m)
            pos, dist = check_bytes(P, T, vals, pt, k, what=("k>=m", m, k))
            assert len(pos) == n - m + 1 and dist.max() == m


def test_foreign_bytes_and_empty_sets_are_counted_into_the_distance():
    vals, n = ACGNT, 4097
    rng = np.random.default_rng(630)
    T = random_text(vals, n, 631)
    T[:5] = vals
    for m in (12, 40):
        P = random_text(vals, m, 632 + m)
        plant(T, 2000, P, 1, vals, rng)
        F = P.copy()
        F[[1, m - 2]] = (200, 201)  # two bytes the text does not hold
        with PackedText.upload(T, wide=True) as pt:
            assert psearch_mis(F, pt, 1)[0] == 0 and pfind_mis(F, pt, 1)[2] == 0  # more foreign bytes than k: no occurrence
            for k in (2, 3, 7):
                pos, dist = check_bytes(F, T, vals, pt, k, what=("foreign", m, k))
                assert (k == 2 or len(pos) > 0) and (dist >= 2).all()
            at = pfind_mis(F, pt, 3)[0].tolist()
            assert 2000 in at
            sets = sets_of(P, vals)
            sets[[0, 5]] = 0
            assert psearch_sets_mis(sets, pt, 1)[0] == 0
            pos, dist = check_sets(sets, T, vals, pt, 3, what=("empty", m))
            assert 2000 in pos.tolist() and dist.min() >= 2


# ---- ranges, cap, batch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vals", [ACGNT, EIGHT])
def test_sub_ranges_that_begin_and_end_mid_dword(vals):
    n = 2**16 + 77
    rng = np.random.default_rng(700 + len(vals))
    T = random_text(vals, n, 701 + len(vals))
    for m in (5, 40):
        P = random_text(vals, m, 702 + m)
        for at in (0, 33, 127, 128, 1000, 8191, 8192 + 13, 30000, n - m):
            plant(T, at, P, int(rng.integers(0, 3)), vals, rng)
        with PackedText.upload(T, wide=True) as pt:
            for off, ln in ((0, n), (1, n - 1), (33, 100), (127, 8192), (129, 8065 + m), (8191, 30000), (8192 + 13, m), (8192 + 14, m),
                            (n - m - 3, m + 3), (n - m, m), (1000, m - 1), (5, 0)):
                check_bytes(P, T, vals, pt, 0, off, ln, what=(vals, m, off, ln))
                check_bytes(P, T, vals, pt, 2, off, ln, what=(vals, m, off, ln, "k=2"))
                check_sets(iupac_like(P, vals, np.random.default_rng(m)), T, vals, pt, 1, off, ln, what=(vals, m, off, ln, "sets"))


def test_a_cap_one_short_is_nomem_with_the_count():
    vals, n = ACGNT, 4097
    T = random_text(vals, n, 710)
    P = T[100:103].copy()
    sets = sets_of(P, vals)
    with PackedText.upload(T, wide=True) as pt:
        want = len(by_definition(sets, T, vals, 0)[0])
        want1 = len(by_definition(sets, T, vals, 1)[0])
        assert want > 2 and want1 > want
        assert pfind(P, pt, cap=want - 1) == (None, want)
        assert pfind_sets(sets, pt, cap=want - 1) == (None, want)
        assert pfind_mis(P, pt, 1, cap=want1 - 1) == (None, None, want1)
        assert pfind_sets_mis(sets, pt, 1, cap=want1 - 1) == (None, None, want1)
        assert pfind(P, pt, cap=0) == (None, want)
        L, c = engine.lib(), ctypes.c_uint64(0)
        out = np.zeros(want, dtype=np.uint64)
        assert L.smartgpu_pfind64(P.ctypes.data, 3, pt._h, 0, n, out.ctypes.data, want - 1, ctypes.byref(c)) == ERR_NOMEM and c.value == want
        assert L.smartgpu_pfind64(P.ctypes.data, 3, pt._h, 0, n, out.ctypes.data, want, ctypes.byref(c)) == 0 and c.value == want


@pytest.mark.parametrize("m", [3, 40])
def test_batch_calls(m):
    vals, n = EIGHT, 2**16 + 5
    T = random_text(vals, n, 720 + m)
    pats = [T[1000 * i + 7:1000 * i + 7 + m].copy() for i in range(12)]
    pats.append(np.full(m, 200, dtype=np.uint8))  # a pattern the text does not hold
    pats.append(pats[0].copy())
    for i in range(3):
        T[40000 + 100 * i:40000 + 100 * i + m] = pats[i]
    with PackedText.upload(T, wide=True) as pt:
        counts, _ = psearch_batch(pats, pt)
        lists, fcounts = pfind_batch(pats, pt, cap=int(counts.sum()))
        for i, P in enumerate(pats):
            wpos = by_definition(sets_of(P, vals), T, vals, 0)[0]
            assert counts[i] == fcounts[i] == len(wpos) and np.array_equal(lists[i], wpos), (m, i)
        assert counts[12] == 0 and counts[0] >= 2
        lists, fcounts = pfind_batch(pats, pt, cap=int(counts.sum()) - 1)
        assert lists is None and np.array_equal(fcounts, counts)
        sub, _ = psearch_batch(pats[:3], pt, off=33, n=40000)
        for i in range(3):
            assert sub[i] == len(by_definition(sets_of(pats[i], vals), T, vals, 0, 33, 40000)[0])


def test_the_batch_bound_is_refused_with_its_message():
    vals = ACGNT
    T = random_text(vals, 4097, 730)
    T[:5] = vals
    pats = [np.array([vals[i % 5]], dtype=np.uint8) for i in range(BATCH_BOUND + 1)]
    with PackedText.upload(T, wide=True) as pt:
        with pytest.raises(smart_amd.SmartGpuError, match=str(BATCH_BOUND)):
            psearch_batch(pats, pt)
        with pytest.raises(smart_amd.SmartGpuError, match=str(BATCH_BOUND)):
            pfind_batch(pats, pt)
        counts, _ = psearch_batch(pats[:BATCH_BOUND], pt)  # the bound itself is served
        for i in range(5):
            assert counts[i] == int((T == vals[i]).sum())
    four = T[T != 78]
    with PackedText.upload(four) as two:  # a two-plane text is not bound by it
        assert two.planes == 2
        counts, _ = psearch_batch([np.array([(65, 67, 71, 84)[i % 4]], dtype=np.uint8) for i in range(BATCH_BOUND + 1)], two)
        assert counts[0] == counts[BATCH_BOUND] == int((four == 65).sum())


# ---- against the existing kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 2**18 + 3])
def test_differential_against_the_two_plane_kernels(n):
    """A text over ACGT with one N appended is a three-plane text; on the range that leaves out the last symbol every call
    must answer what it answers on the two-plane text of the same symbols."""
    rng = np.random.default_rng(800 + n)
    base = random_text((65, 67, 71, 84), n, 801 + n)
    wide_T = np.concatenate([base, np.array([78], dtype=np.uint8)])

    def wide_sets(s4):  # sets over ACGT (T = bit 3) as sets over ACGNT (T = bit 4)
        s4 = np.asarray(s4, dtype=np.uint8)
        return ((s4 & 7) | ((s4 & 8) << 1)).astype(np.uint8)

    with PackedText.upload(wide_T, wide=True) as w, PackedText.upload(base) as two:
        assert w.planes == 3 and two.planes == 2 and w.symbols() == list(ACGNT)
        for m in (1, 8, 32, 33, 65, 200):
            P = base[n // 2:n // 2 + m].copy()
            Q = base[n // 4:n // 4 + m].copy()  # a near copy of another window
            Q[m // 2] = other_value((65, 67, 71, 84), Q[m // 2], rng)
            s4 = (1 << np.searchsorted(np.array([65, 67, 71, 84], dtype=np.uint8), P)).astype(np.uint8)
            s4 |= (rng.random(m) < 0.3).astype(np.uint8) << rng.integers(0, 4, m).astype(np.uint8)
            for off, ln in ((0, n), (37, n - 37 - 29)):
                if m > ln:
                    continue
                for pat in (P, Q):
                    assert psearch(pat, w, off=off, n=ln)[0] == psearch(pat, two, off=off, n=ln)[0]
                    a, b = pfind(pat, w, off=off, n=ln), pfind(pat, two, off=off, n=ln)
                    assert a[1] == b[1] and np.array_equal(a[0], b[0])
                    for k in (1, 3, 7):
                        assert psearch_mis(pat, w, k, off=off, n=ln)[0] == psearch_mis(pat, two, k, off=off, n=ln)[0]
                        a, b = pfind_mis(pat, w, k, off=off, n=ln, cap=1 << 19), pfind_mis(pat, two, k, off=off, n=ln, cap=1 << 19)
                        assert a[2] == b[2] and (a[0] is None) == (b[0] is None)
                        if a[0] is not None:
                            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                assert psearch_sets(wide_sets(s4), w, off=off, n=ln)[0] == psearch_sets(s4, two, off=off, n=ln)[0] > 0
                a, b = pfind_sets(wide_sets(s4), w, off=off, n=ln), pfind_sets(s4, two, off=off, n=ln)
                assert a[1] == b[1] and np.array_equal(a[0], b[0])
                for k in (1, 4):
                    a = pfind_sets_mis(wide_sets(s4), w, k, off=off, n=ln, cap=1 << 19)
                    b = pfind_sets_mis(s4, two, k, off=off, n=ln, cap=1 << 19)
                    assert a[2] == b[2] == psearch_sets_mis(wide_sets(s4), w, k, off=off, n=ln)[0]
                    if a[0] is not None:
                        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            counts_w, _ = psearch_batch([P, Q], w, n=n)
            counts_2, _ = psearch_batch([P, Q], two)
            assert np.array_equal(counts_w, counts_2)


SEED = 20261019


def fuzz_text(vals, n, kind, rng):
    v = np.asarray(vals, dtype=np.uint8)
    if kind == 0:
        return v[rng.integers(0, len(v), n)]
    if kind == 1:  # skewed
        p = np.array([0.6] + [0.4 / (len(v) - 1)] * (len(v) - 1))
        return v[rng.choice(len(v), size=n, p=p)]
    runs = rng.integers(1, 40, n // 8 + 2)  # run-heavy
    return np.resize(np.repeat(v[rng.integers(0, len(v), len(runs))], runs), n)


def test_seeded_differential_loop():
    """200 seeded cases: 5 to 8 values, m <= 300, random k, sets or bytes, uniform, skewed and run-heavy texts up to
    2^18 + 77 symbols (most are short: the numpy reference is the slow side).  A failure names seed and case."""
    rng = np.random.default_rng(SEED)
    texts = []
    for t in range(10):
        nv = int(rng.integers(5, 9))
        vals = tuple(sorted(rng.choice(256, size=nv, replace=False).tolist()))
        n = 2**18 + 77 if t == 0 else int(rng.integers(700, 20000))
        T = fuzz_text(vals, n, t % 3, rng)
        T[:nv] = vals
        texts.append((vals, T))
    case = 0
    for vals, T in texts:
        n = len(T)
        with PackedText.upload(T, wide=True) as pt:
            assert pt.planes == 3 and pt.symbols() == list(vals), (SEED, case)
            for _ in range(20):
                m = int(rng.integers(1, 301))
                k = int(rng.integers(0, 8))
                at = int(rng.integers(0, n - m + 1))
                W = T[at:at + m].copy()
                for j in rng.choice(m, size=min(m, int(rng.integers(0, k + 2))), replace=False):
                    W[j] = other_value(vals, W[j], rng)
                off = int(rng.integers(0, 200)) if rng.random() < 0.5 else 0
                ln = n - off - (int(rng.integers(0, 200)) if rng.random() < 0.5 else 0)
                what = "seed %d case %d (values %s, n %d, m %d, k %d, range %d+%d)" % (SEED, case, vals, n, m, k, off, ln)
                if rng.random() < 0.5:
                    if rng.random() < 0.3:
                        W[int(rng.integers(0, m))] = next(x for x in range(256) if x not in vals)  # a foreign byte
                    check_bytes(W, T, vals, pt, k, off, ln, what=what)
                    if k:
                        check_bytes(W, T, vals, pt, 0, off, ln, what=what + " k=0")
                else:
                    sets = iupac_like(W, vals, rng, extra=float(rng.choice([0.05, 0.3, 0.7])))
                    if rng.random() < 0.2:
                        sets[int(rng.integers(0, m))] = 0
                    check_sets(sets, T, vals, pt, k, off, ln, what=what)
                    if k:
                        check_sets(sets, T, vals, pt, 0, off, ln, what=what + " k=0")
                case += 1
    assert case == 200


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_a_set_bit_at_or_above_the_number_of_values_is_refused():
    T = random_text(ACGNT, 4097, 900)
    T[:5] = ACGNT
    with PackedText.upload(T, wide=True) as pt:
        ok = np.array([1, 16, 31, 8], dtype=np.uint8)  # bits up to nvalues - 1 = 4 are served
        assert psearch_sets(ok, pt)[0] == len(by_definition(ok, T, ACGNT, 0)[0])
        bad = np.array([1, 16, 32, 64], dtype=np.uint8)
        for call in (lambda: psearch_sets(bad, pt), lambda: pfind_sets(bad, pt), lambda: psearch_sets_mis(bad, pt, 2), lambda: pfind_sets_mis(bad, pt, 2)):
            with pytest.raises(smart_amd.SmartGpuError, match="position 2"):
                call()


def test_edit_and_align_calls_refuse_a_three_plane_text():
    T = random_text(ACGNT, 4097, 910)
    T[:5] = ACGNT
    P = T[100:120].copy()
    sets = sets_of(P, ACGNT)
    ends = np.array([150], dtype=np.uint64)
    with PackedText.upload(T, wide=True) as pt:
        calls = [lambda: smart_amd.psearch_edit(P, pt, 2), lambda: smart_amd.pfind_edit(P, pt, 2), lambda: smart_amd.psearch_sets_edit(sets, pt, 2),
                 lambda: smart_amd.pfind_sets_edit(sets, pt, 2), lambda: smart_amd.psearch_editl(P, pt, 2), lambda: smart_amd.pfind_editl(P, pt, 2),
                 lambda: smart_amd.psearch_sets_editl(sets, pt, 2), lambda: smart_amd.pfind_sets_editl(sets, pt, 2),
                 lambda: smart_amd.palign_edit(P, pt, 2, ends), lambda: smart_amd.palign_sets_edit(sets, pt, 2, ends)]
        for call in calls:
            with pytest.raises(smart_amd.SmartGpuError, match="three-plane texts .* are not offered"):
                call()
        L, c = engine.lib(), ctypes.c_uint64(77)
        assert L.smartgpu_psearch_edit64(P.ctypes.data, 20, 2, pt._h, 0, 4097, ctypes.byref(c), None, None) == ERR_ARG and c.value == 77
        assert L.smartgpu_psearch_editl64(P.ctypes.data, 20, 2, 0, pt._h, 0, 4097, ctypes.byref(c), None, None) == ERR_ARG and c.value == 77
        st = np.zeros(1, dtype=np.uint64)
        assert L.smartgpu_palign_edit64(P.ctypes.data, 20, 2, pt._h, 0, 4097, ends.ctypes.data, 1, st.ctypes.data, None, None) == ERR_ARG
        assert "not offered" in L.smartgpu_last_error().decode()
