"""Set patterns with up to k mismatches on packed texts on the GPU (planes_sets_mis_scan, planes_sets_mis_find): counts,
positions and distances against the DEFINITION, computed here with numpy — the distance of start position s is the number
of j < m for which the code of T[s + j] is not a member of sets[j], and s is an occurrence when it is at most k.  Every
comparison is exact equality; no text is longer than 2^20 + 3 symbols.  Every case asserts, from the definition alone, that
what it expects is not empty."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (PackedText, iupac_revcomp, iupac_sets, pfind_mis, pfind_sets, pfind_sets_mis, psearch_mis, psearch_sets,  # noqa: E402
                       psearch_sets_mis)

from test_packed_text_gpu import MS  # noqa: E402

ACGT = (65, 67, 71, 84)
GRID_VALUES = [ACGT, (0, 255), (65, 67, 84)]
GRID_NS = [33, 4097, 2**20 + 3]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def random_text(vals, n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]


def codes_of(T, vals):
    """The code of every symbol: the rank of its byte among the text's values."""
    return np.searchsorted(np.asarray(sorted(vals), dtype=np.uint8), T).astype(np.uint8)


def singletons(T, vals):
    return (1 << codes_of(T, vals)).astype(np.uint8)


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
    miss = [np.array([not (int(x) >> c) & 1 for c in range(4)], dtype=np.uint8) for x in sets]  # miss[j][code]
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


def check(sets, T, vals, pt, k, off=0, n=None, what=None):
    """Count, positions and distances of both calls against the definition; returns (positions, distances)."""
    sets = np.asarray(sets, dtype=np.uint8)
    wpos, wdist = by_definition(sets, T, vals, k, off, n)
    got = psearch_sets_mis(sets, pt, k, off=off, n=n)[0]
    assert got == len(wpos), (what, got, len(wpos))
    pos, dist, cnt = pfind_sets_mis(sets, pt, k, off=off, n=n, cap=max(len(wpos), 1))
    assert cnt == len(wpos) and pos is not None and pos.dtype == np.uint64 and dist.dtype == np.uint8, (what, cnt, len(wpos))
    assert np.array_equal(pos, wpos), what
    assert np.array_equal(dist, wdist), what
    return pos, dist


def iupac_like(window, vals, rng, extra=0.3):
    """Sets that accept `window`: the singleton of each of its symbols, with every other code added with probability `extra`."""
    s = singletons(window, vals)
    for c in range(len(vals)):
        s |= ((rng.random(len(window)) < extra).astype(np.uint8) << c).astype(np.uint8)
    return s


def other_code(vals, c, rng=None):
    rest = [x for x in range(len(vals)) if x != c]
    return rest[0] if rng is None else int(rng.choice(rest))


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vals", GRID_VALUES)
@pytest.mark.parametrize("n", GRID_NS)
def test_k0_is_the_set_matcher(vals, n):
    T = random_text(vals, n, 9000 + n + len(vals))
    rng = np.random.default_rng(9100 + n + len(vals))
    checked = 0
    with PackedText.upload(T) as pt:
        for m in MS:
            if m > n:
                continue
            mid = (n - m) // 2
            sets = iupac_like(T[mid:mid + m], vals, rng)
            want = psearch_sets(sets, pt)[0]
            wpos, wcnt = pfind_sets(sets, pt, cap=max(want, 1))
            pos, dist = check(sets, T, vals, pt, 0, what=(vals, n, m))
            assert mid in pos.tolist(), (vals, n, m)  # by the definition: the window the sets were cut from
            assert len(pos) == want == wcnt and np.array_equal(pos, wpos) and not dist.any(), (vals, n, m)
            checked += 1
    assert checked >= 2


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("vals", GRID_VALUES)
@pytest.mark.parametrize("n", GRID_NS)
def test_singleton_sets_are_the_mismatch_matcher(vals, n, k):
    T = random_text(vals, n, 9200 + n + len(vals))
    rng = np.random.default_rng(9300 + n + len(vals) + 17 * k)
    byte_of = np.asarray(sorted(vals), dtype=np.uint8)
    total, far = 0, 0
    with PackedText.upload(T) as pt:
        for m in MS:
            if m > n:
                continue
            c = int(rng.integers(0, n - m + 1))
            code = codes_of(T[c:c + m], vals)
            for j in rng.choice(m, size=min(m, int(rng.integers(0, k + 1))), replace=False):
                code[j] = other_code(vals, code[j], rng)
            P = byte_of[code]
            sets = (1 << code).astype(np.uint8)
            pos, dist = check(sets, T, vals, pt, k, what=(vals, n, m, k))
            assert c in pos.tolist(), (vals, n, m, k)  # at most k positions of the cut window were changed
            assert psearch_mis(P, pt, k)[0] == len(pos), (vals, n, m, k)
            mpos, mdist, mcnt = pfind_mis(P, pt, k, cap=max(len(pos), 1))
            assert mcnt == len(pos) and np.array_equal(mpos, pos) and np.array_equal(mdist, dist), (vals, n, m, k)
            total += len(pos)
            far += int((dist > 0).sum())
    assert total > 0 and far > 0


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_every_set_at_every_position(vals):
    """m = 40: each of the first 32 positions (the switch and the counter) and the verification beyond (both levels of the
    multiplexer), each proper non-empty set, once with the cut window's symbol a member and once not."""
    n, m = 4097, 40
    T = random_text(vals, n, 9400 + len(vals))
    code = codes_of(T, vals)
    proper = range(1, (1 << len(vals)) - 1)
    assert len(proper) == (14 if len(vals) == 4 else 2)
    with PackedText.upload(T) as pt:
        for j in range(m):
            for s in proper:
                member = (s >> code[1000 + j:3000 + j]) & 1
                cut_in = 1000 + int(np.flatnonzero(member == 1)[0])
                cut_out = 1000 + int(np.flatnonzero(member == 0)[0])
                # the symbol is a member: distance 0 at the cut, found with k = 0
                sets = singletons(T[cut_in:cut_in + m], vals)
                sets[j] = s
                pos, dist = check(sets, T, vals, pt, 0, what=(vals, j, s, "in"))
                at = np.flatnonzero(pos == cut_in)
                assert len(at) == 1 and dist[at[0]] == 0, (vals, j, s)
                # it is not: distance 1, absent with k = 0, present with k = 1
                sets = singletons(T[cut_out:cut_out + m], vals)
                sets[j] = s
                assert by_definition(sets, T, vals, 1)[0].tolist().count(cut_out) == 1
                pos0, _ = check(sets, T, vals, pt, 0, what=(vals, j, s, "out", 0))
                assert cut_out not in pos0.tolist(), (vals, j, s)
                pos, dist = check(sets, T, vals, pt, 1, what=(vals, j, s, "out", 1))
                at = np.flatnonzero(pos == cut_out)
                assert len(at) == 1 and dist[at[0]] == 1, (vals, j, s)


# 4 ---------------------------------------------------------------------------------------------------------------------
def two_member_sets(m, rng):
    a = rng.integers(0, 4, m)
    b = (a + rng.integers(1, 4, m)) % 4
    return ((1 << a) | (1 << b)).astype(np.uint8)


def instance_of(sets, rng, wrong=()):
    """Codes of a window in which exactly the positions `wrong` hold a non-member of their (proper, non-empty) set."""
    code = np.zeros(len(sets), dtype=np.uint8)
    wrong = set(int(j) for j in wrong)
    for j, s in enumerate(sets):
        pool = [c for c in range(4) if bool(int(s) >> c & 1) != (j in wrong)]
        code[j] = rng.choice(pool)
    return code


@pytest.mark.parametrize("m", [8, 33, 100, 4200])
def test_budget_boundary(m):
    """Windows planted with exactly d = 0 .. 9 non-member positions, in the first 32 positions only, beyond them only, or split."""
    n = 2**16 + 5
    rng = np.random.default_rng(9500 + m)
    byte_of = np.asarray(ACGT, dtype=np.uint8)
    for where in ("first", "beyond", "split"):
        if where != "first" and m <= 32:
            continue
        T = random_text(ACGT, n, 9600 + m)
        sets = two_member_sets(m, rng)
        planted = []
        for d in range(10):
            if where == "first":
                pool, parts = [np.arange(min(m, 32))], [d]
            elif where == "beyond":
                pool, parts = [np.arange(32, m)], [d]
            else:
                pool, parts = [np.arange(32), np.arange(32, m)], [d // 2, d - d // 2]
            if any(c > len(p) for c, p in zip(parts, pool)):
                continue
            at = 77 + d * (m + 131)
            wrong = np.concatenate([rng.choice(p, size=c, replace=False) for c, p in zip(parts, pool)])
            T[at:at + m] = byte_of[instance_of(sets, rng, wrong)]
            planted.append((at, d))
        assert planted and planted[0][1] == 0 and planted[-1][0] + m <= n
        with PackedText.upload(T) as pt:
            for k in range(8):
                pos, dist = check(sets, T, ACGT, pt, k, what=(m, where, k))
                found = dict(zip(pos.tolist(), dist.tolist()))
                for at, d in planted:
                    assert found.get(at) == (d if d <= k else None), (m, where, k, at, d)


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [8, 9, 16, 17, 64, 256, 257, 4200])
def test_saturation(m):
    """{C, G} at every position against a long stretch of A: every window there has m non-members.  A counter that wraps
    passes at 8, 16 and 256; the sticky bit does not."""
    n, stretch = 2**16 + 5, 2**16 - 5000
    T = np.full(n, 65, dtype=np.uint8)
    T[stretch:] = random_text(ACGT, n - stretch, 9700 + m)
    T[stretch + 100:stretch + 100 + m] = random_text((67, 71), m, 9710 + m)  # an occurrence at distance 0 behind the stretch
    sets = np.full(m, 0b0110, dtype=np.uint8)
    with PackedText.upload(T) as pt:
        for k in range(8):
            if k >= m:
                continue
            pos, _ = check(sets, T, ACGT, pt, k, what=(m, k))
            assert stretch + 100 in pos.tolist()
            assert not (pos + m <= stretch).any(), (m, k)


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vals", [ACGT, (65, 67, 84), (0, 255)])
@pytest.mark.parametrize("g", [1, 2, 3])
def test_full_sets_cost_no_budget(vals, g):
    n, cut = 2**16 + 5, 40000
    T = random_text(vals, n, 9800 + len(vals))
    full = (1 << len(vals)) - 1
    with PackedText.upload(T) as pt:
        for m, places in ((8, [1, 4, 7][:g]), (40, [5, 33, 38][:g]), (40, [3, 17, 31][:g]), (100, [64, 65, 99][:g])):
            sets = singletons(T[cut:cut + m], vals)
            sets[places] = full
            pos, dist = check(sets, T, vals, pt, 0, what=(vals, g, m))
            at = np.flatnonzero(pos == cut)
            assert len(at) == 1 and dist[at[0]] == 0, (vals, g, m)
            assert len(pos) == psearch_sets(sets, pt)[0]


@pytest.mark.parametrize("u", [1, 2, 3])
def test_empty_sets(u):
    """A position with the empty set is a mismatch in every window: not 0 occurrences, as the set calls answer."""
    n, cut = 2**16 + 5, 40000
    T = random_text(ACGT, n, 9900)
    with PackedText.upload(T) as pt:
        for m, places in ((40, ([3, 17, 31][:u], [32, 35, 39][:u], [5, 33, 38][:u])), (100, ([0, 31, 32][:u], [64, 65, 99][:u]))):
            for at in places:
                sets = singletons(T[cut:cut + m], ACGT)
                sets[at] = 0
                assert psearch_sets(sets, pt)[0] == 0
                for k in (u - 1, u, u + 2):
                    pos, dist = check(sets, T, ACGT, pt, k, what=(u, m, at, k))
                    if k == u - 1:
                        assert len(pos) == 0
                        cnt, pre_ms, run_ms = psearch_sets_mis(sets, pt, k)
                        assert (cnt, pre_ms, run_ms) == (0, 0.0, 0.0)  # decided on the host: nothing was staged or launched
                    else:
                        i = np.flatnonzero(pos == cut)
                        assert len(i) == 1 and dist[i[0]] == u and dist.min() >= u, (u, m, at, k)


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vals", [(0, 1), ACGT, (3, 200, 255)])
@pytest.mark.parametrize("n", [1000 + 13, 4097, 33, 95])
def test_the_pad_is_not_text(vals, n):
    """The zero pad around the planes looks like the lowest value, which every set here accepts: a window reaching into it
    would be an occurrence."""
    assert n % 32 != 0
    T = random_text(vals, n, 10000 + n)
    tail = min(n // 2, 300)
    T[n - tail:] = min(vals)
    T[:tail] = min(vals)
    T[tail] = vals[1]
    vals = tuple(sorted(set(T.tolist())))  # the values the text HOLDS (a short text may lack some): the codes are their ranks
    assert len(vals) >= 2
    top = 1 << (len(vals) - 1)
    checked = 0
    with PackedText.upload(T) as pt:
        for m in (1, 2, 5, 31, 32, 33, 64, 100, 257):
            if m > tail:
                continue
            sets = np.full(m, 1, dtype=np.uint8)
            sets[1::2] |= top  # the lowest code alone, and with the highest
            for k in (1, 3, 7):
                for off in (0, 1, 31, 32, 33):
                    if off + m > n:
                        continue
                    pos, _ = check(sets, T, vals, pt, k, off=off, what=(n, m, k, off))
                    assert len(pos) > 0
                    pos, _ = check(sets, T, vals, pt, k, off=off, n=min(n - off, tail + 3), what=(n, m, k, off, "short"))
                    assert len(pos) > 0
                    checked += 1
    assert checked > 0


# 8 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_text():
    n = 2**17 + 77
    T = random_text(ACGT, n, 10100)
    T[60000:70000] = 65  # a run across 65536: dense survivors around the borders
    return T


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("m", [1, 3, 32, 40])
def test_sub_ranges(run_text, m, k):
    T = run_text
    n = len(T)
    sets = np.full(m, 0b0001, dtype=np.uint8)
    sets[1::2] = 0b0101  # A, and A or G
    total = 0
    with PackedText.upload(T) as pt:
        edges = sorted({b + d for b in (0, 32, 128, 8192, 65536) for d in (-1, 0, 1) if b + d >= 0})
        for off in edges:
            for end in edges + [n]:
                if end < off:
                    continue
                total += len(check(sets, T, ACGT, pt, k, off=off, n=end - off, what=(m, k, off, end))[0])
        long = np.full(100, 0b0101, dtype=np.uint8)
        assert psearch_sets_mis(long, pt, k, off=10, n=50)[0] == 0  # m > n
        pos, dist, cnt = pfind_sets_mis(long, pt, k, off=10, n=50)
        assert cnt == 0 and len(pos) == 0 and len(dist) == 0
    assert total > 0


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_a_primer_on_both_strands():
    primer = "GGNCCWRTATAWAW"
    n, m, k = 2**20 + 3, len(primer), 2
    rng = np.random.default_rng(10200)
    T = random_text(ACGT, n, 10201)
    byte_of = np.asarray(ACGT, dtype=np.uint8)
    strands = (primer, iupac_revcomp(primer))
    assert strands[1] == "WTWTATAYWGGNCC"
    planted = {}
    for si, pattern in enumerate(strands):
        sets = iupac_sets(pattern, ACGT)
        proper = np.flatnonzero(sets != 15)
        planted[si] = []
        for d in range(4):
            at = 1000 + 65536 * (4 * si + d) + 31 * d
            T[at:at + m] = byte_of[instance_of(sets, rng, rng.choice(proper, size=d, replace=False))]
            planted[si].append((at, d))
    with PackedText.upload(T) as pt:
        assert pt.symbols() == list(ACGT)
        for si, pattern in enumerate(strands):
            sets = pt.iupac(pattern)
            pos, dist = check(sets, T, ACGT, pt, k, what=pattern)
            found = dict(zip(pos.tolist(), dist.tolist()))
            for at, d in planted[si]:
                assert found.get(at) == (d if d <= k else None), (pattern, at, d)
            assert (dist > 0).any()


# 10 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 7])
def test_k_at_least_m(m):
    n = 5003
    T = random_text(ACGT, n, 10300 + m)
    sets = two_member_sets(m, np.random.default_rng(10310 + m))
    with PackedText.upload(T) as pt:
        pos, dist = check(sets, T, ACGT, pt, 7, what=m)
        assert len(pos) == n - m + 1 and np.array_equal(pos, np.arange(n - m + 1, dtype=np.uint64))
        assert dist.max() <= m and dist.max() > 0 and dist.min() == 0


# 11 --------------------------------------------------------------------------------------------------------------------
def test_host_decisions():
    L = smart_amd.lib()
    T = random_text(ACGT, 5000, 10400)
    sets = np.asarray([0b0011, 0b0100, 0b1010, 0b0001], dtype=np.uint8)
    with PackedText.upload(T) as pt:
        wpos, wdist = by_definition(sets, T, ACGT, 1)
        assert len(wpos) > 10 and (wdist > 0).any()
        # cap smaller than the count: SMARTGPU_ERR_NOMEM with count filled; cap = 0 with no buffer is a count
        out = np.zeros(4, dtype=np.uint64)
        mis = np.zeros(4, dtype=np.uint8)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_sets_mis64(sets.ctypes.data, 4, 1, pt._h, 0, len(T), out.ctypes.data, mis.ctypes.data, 4, ctypes.byref(c)) == -5
        assert c.value == len(wpos)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_sets_mis64(sets.ctypes.data, 4, 1, pt._h, 0, len(T), None, None, 0, ctypes.byref(c)) == -5
        assert c.value == len(wpos)
        # mismatches NULL with positions given
        out = np.zeros(len(wpos), dtype=np.uint64)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_sets_mis64(sets.ctypes.data, 4, 1, pt._h, 0, len(T), out.ctypes.data, None, len(out), ctypes.byref(c)) == 0
        assert c.value == len(wpos) and np.array_equal(out, wpos)
        assert pfind_sets_mis(sets, pt, 1, cap=4) == (None, None, len(wpos))
        assert pfind_sets_mis(sets, pt, 1, cap=0) == (None, None, len(wpos))
        # nothing within the budget: a count of 0 needs no room
        never = np.zeros(12, dtype=np.uint8)
        c = ctypes.c_uint64(9)
        assert L.smartgpu_pfind_sets_mis64(never.ctypes.data, 12, 7, pt._h, 0, len(T), None, None, 0, ctypes.byref(c)) == 0 and c.value == 0
        with pytest.raises(smart_amd.SmartGpuError):
            psearch_sets_mis(sets, pt, 8)
        with pytest.raises(smart_amd.SmartGpuError):
            pfind_sets_mis(sets, pt, 1, off=4000, n=2000)  # a range outside the text
    # a set with a bit at or above the text's number of values: refused, the position named, nothing written
    T3 = random_text((65, 67, 84), 5000, 10401)
    bad = np.asarray([0b0001, 0b0011, 0b1001, 0b0111], dtype=np.uint8)
    with PackedText.upload(T3) as pt:
        c = ctypes.c_uint64(77)
        assert L.smartgpu_psearch_sets_mis64(bad.ctypes.data, 4, 1, pt._h, 0, len(T3), ctypes.byref(c), None, None) == -3
        msg = L.smartgpu_last_error().decode()
        assert "position 2" in msg and c.value == 77, msg
        c = ctypes.c_uint64(77)
        assert L.smartgpu_pfind_sets_mis64(bad.ctypes.data, 4, 1, pt._h, 0, len(T3), None, None, 0, ctypes.byref(c)) == -3
        assert "position 2" in L.smartgpu_last_error().decode() and c.value == 77
        bad[2] = 0b0101
        assert psearch_sets_mis(bad, pt, 1)[0] == len(by_definition(bad, T3, (65, 67, 84), 1)[0]) > 0
