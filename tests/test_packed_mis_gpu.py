"""Occurrences with up to k mismatches on packed texts on the GPU (planes_mis_scan, planes_mis_find): counts, positions and
distances against the DEFINITION, computed here with numpy — start position s is an occurrence when the number of j < m
with T[s + j] != P[j] is at most k.  Every comparison is exact equality; no text is longer than 2^20 + 3 symbols."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import PackedText, pfind, pfind_mis, psearch, psearch_mis  # noqa: E402

from test_packed_text_gpu import MS, VALUE_SETS  # noqa: E402

ACGT = (65, 67, 71, 84)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def random_text(vals, n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]


def by_definition(P, T, k, off=0, n=None):
    """(ascending start positions relative to symbol 0 as uint64, their distances as uint8) in [off, off + n - m]: a
    progressive filter — the candidates' running mismatch counts, candidates dropped once they are over k."""
    n = len(T) - off if n is None else n
    m = len(P)
    if m > n:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    s = np.arange(off, off + n - m + 1, dtype=np.int64)
    d = np.zeros(len(s), dtype=np.int32)
    for j in range(m):
        d += T[s + j] != P[j]
        keep = d <= k
        if not keep.all():
            s, d = s[keep], d[keep]
            if len(s) == 0:
                break
    return s.astype(np.uint64), d.astype(np.uint8)


def check(P, T, pt, k, off=0, n=None, what=None):
    """Count, positions and distances of both calls against the definition; returns (positions, distances)."""
    P = np.asarray(P, dtype=np.uint8)
    wpos, wdist = by_definition(P, T, k, off, n)
    got = psearch_mis(P, pt, k, off=off, n=n)[0]
    assert got == len(wpos), (what, got, len(wpos))
    pos, dist, cnt = pfind_mis(P, pt, k, off=off, n=n, cap=max(len(wpos), 1))
    assert cnt == len(wpos) and pos is not None and pos.dtype == np.uint64 and dist.dtype == np.uint8, (what, cnt, len(wpos))
    assert np.array_equal(pos, wpos), what
    assert np.array_equal(dist, wdist), what
    return pos, dist


def other(vals, v):
    return next(x for x in vals if x != v)


@pytest.mark.parametrize("vals", VALUE_SETS)
@pytest.mark.parametrize("n", [33, 4097, 2**20 + 3])
def test_k0_is_the_exact_matcher(vals, n):
    T = random_text(vals, n, 2000 + n)
    checked = 0
    with PackedText.upload(T) as pt:
        for m in MS:
            if m > n:
                continue
            mid = (n - m) // 2
            pats = [T[mid:mid + m]]
            if len(vals) > 1:  # the same with one symbol changed to another value of the text
                P = T[mid:mid + m].copy()
                P[m // 2] = other(vals, P[m // 2])
                pats.append(P)
            for P in pats:
                want = psearch(P, pt)[0]
                assert psearch_mis(P, pt, 0)[0] == want, (vals, n, m)
                wpos, wcnt = pfind(P, pt, cap=max(want, 1))
                gpos, gdist, gcnt = pfind_mis(P, pt, 0, cap=max(want, 1))
                assert gcnt == wcnt == want and np.array_equal(gpos, wpos) and not gdist.any(), (vals, n, m)
                checked += 1
    assert checked >= 2


@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_one_planted_mismatch_at_every_pattern_position(vals):
    """m = 40: each of the first 32 positions (the counter) and the verification beyond."""
    n, m, cut = 4097, 40, 1234
    T = random_text(vals, n, 100 + len(vals))
    with PackedText.upload(T) as pt:
        for j in range(m):
            P = T[cut:cut + m].copy()
            P[j] = other(vals, P[j])
            pos, dist = check(P, T, pt, 1, what=(vals, j, 1))
            at = np.flatnonzero(pos == cut)
            assert len(at) == 1 and dist[at[0]] == 1, (vals, j)
            pos0, _ = check(P, T, pt, 0, what=(vals, j, 0))
            assert cut not in pos0.tolist(), (vals, j)


@pytest.mark.parametrize("m", [8, 33, 100, 4200])
def test_budget_boundary(m):
    """Windows planted with exactly d = 0 .. 9 mismatches, in the first 32 positions only, beyond them only, or split."""
    n = 2**16 + 5
    rng = np.random.default_rng(500 + m)
    for where in ("first", "beyond", "split"):
        if where != "first" and m <= 32:
            continue
        T = random_text(ACGT, n, 600 + m)
        P = random_text(ACGT, m, 700 + m)
        planted = []
        for d in range(10):
            if where == "first":
                pool = [np.arange(min(m, 32))]
                parts = [d]
            elif where == "beyond":
                pool = [np.arange(32, m)]
                parts = [d]
            else:
                pool = [np.arange(32), np.arange(32, m)]
                parts = [d // 2, d - d // 2]
            if any(c > len(p) for c, p in zip(parts, pool)):
                continue
            at = 77 + d * (m + 131)
            W = P.copy()
            for c, p in zip(parts, pool):
                for j in rng.choice(p, size=c, replace=False):
                    W[j] = other(ACGT, W[j])
            T[at:at + m] = W
            planted.append((at, d))
        assert planted[-1][0] + m <= n
        with PackedText.upload(T) as pt:
            for k in range(8):
                pos, dist = check(P, T, pt, k, what=(m, where, k))
                found = dict(zip(pos.tolist(), dist.tolist()))
                for at, d in planted:
                    assert found.get(at) == (d if d <= k else None), (m, where, k, at, d)


@pytest.mark.parametrize("m", [8, 9, 16, 17, 64, 256, 257, 4200])
def test_saturation(m):
    """C...C against a long stretch of A: every window there has m mismatches.  A counter that wraps passes at 8, 16 and
    256 mismatches; the sticky bit does not."""
    n, stretch = 2**16 + 5, 2**16 - 300
    T = np.full(n, 65, dtype=np.uint8)
    T[stretch:] = random_text((65, 67), n - stretch, 800 + m)
    P = np.full(m, 67, dtype=np.uint8)
    with PackedText.upload(T) as pt:
        for k in range(8):
            if k >= m:
                continue
            pos, _ = check(P, T, pt, k, what=(m, k))
            assert not (pos + m <= stretch).any(), (m, k)


RANDOM_MS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 1000, 4200]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("vals", [ACGT, (0, 255), (65, 67, 84)])
@pytest.mark.parametrize("n", [1000, 2**16 + 5, 2**20 + 3])
def test_random_against_the_definition(vals, n, k):
    T = random_text(vals, n, 3000 + n + len(vals))
    rng = np.random.default_rng(3100 + n + len(vals) + 17 * k)
    total = 0
    with PackedText.upload(T) as pt:
        for m in RANDOM_MS:
            if m > n:
                continue
            c = int(rng.integers(0, n - m + 1))
            P = T[c:c + m].copy()
            for j in rng.choice(m, size=min(m, int(rng.integers(0, k + 2))), replace=False):
                P[j] = other(vals, P[j])
            total += len(check(P, T, pt, k, what=(vals, n, m, k))[0])
    # the cut window itself qualifies whenever its mutations are <= k: with these seeds that holds for some m in every
    # case of the grid, so every case's total — and with it the grid's — is positive by the definition alone
    assert total > 0


@pytest.mark.parametrize("vals", [(0, 1), ACGT])
@pytest.mark.parametrize("unit_len", [1, 2, 3, 4, 5, 6, 7])
def test_periodic_and_one_value_texts(unit_len, vals):
    """Many survivors per lane, dense output, a wave summation for nearly every position."""
    n = 2**16 + 5
    rng = np.random.default_rng(4000 + unit_len + len(vals))
    unit = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), unit_len)]
    T = np.resize(unit, n)
    with PackedText.upload(T) as pt:
        for m in (8, 33, 100, 4200):
            changed = T[:m].copy()
            changed[::50] = [other(vals, v) for v in changed[::50]]
            for P in (T[:m], T[1:1 + m], changed):
                for k in ((2, 7) if m <= 100 else (6,)):
                    check(P, T, pt, k, what=(unit.tolist(), m, k))


@pytest.mark.parametrize("vals", [(0, 1), ACGT, (3, 200, 255)])
@pytest.mark.parametrize("n", [1000 + 13, 4097, 33, 95])
def test_the_pad_is_not_text(vals, n):
    """The zero pad around the planes looks like the lowest value: a window reaching into it would match within the budget."""
    assert n % 32 != 0
    T = random_text(vals, n, 5000 + n)
    tail = min(n // 2, 300)
    T[n - tail:] = min(vals)
    T[:tail] = min(vals)
    T[tail] = vals[1]
    with PackedText.upload(T) as pt:
        for m in (1, 2, 5, 31, 32, 33, 64, 100, 257):
            if m > tail:
                continue
            P = np.full(m, min(vals), dtype=np.uint8)
            for k in (1, 3, 7):
                for off in (0, 1, 31, 32, 33):
                    if off + m > n:
                        continue
                    check(P, T, pt, k, off=off, what=(n, m, k, off))
                    check(P, T, pt, k, off=off, n=min(n - off, tail + 3), what=(n, m, k, off, "short"))


@pytest.fixture(scope="module")
def run_text():
    n = 2**17 + 77
    T = random_text(ACGT, n, 6000)
    T[60000:70000] = 65  # a run across 65536: dense survivors around the borders
    return T


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("m", [1, 3, 32, 40])
def test_sub_ranges(run_text, m, k):
    T = run_text
    n = len(T)
    P = np.full(m, 65, dtype=np.uint8)
    with PackedText.upload(T) as pt:
        edges = sorted({b + d for b in (0, 32, 128, 8192, 65536) for d in (-1, 0, 1) if b + d >= 0})
        for off in edges:
            for end in edges + [n]:
                if end < off:
                    continue
                check(P, T, pt, k, off=off, n=end - off, what=(m, k, off, end))
        long = np.full(100, 65, dtype=np.uint8)
        assert psearch_mis(long, pt, k, off=10, n=50)[0] == 0  # m > n
        pos, dist, cnt = pfind_mis(long, pt, k, off=10, n=50)
        assert cnt == 0 and len(pos) == 0 and len(dist) == 0


@pytest.mark.parametrize("u", [1, 2, 3])
def test_foreign_bytes(u):
    """A pattern byte the text does not hold is a mismatch in every window: not 0 occurrences, as the exact calls answer."""
    n = 2**16 + 5
    T = random_text(ACGT, n, 7100)
    cut = 40000
    with PackedText.upload(T) as pt:
        for m, places in ((40, ([3, 17, 31][:u], [32, 35, 39][:u], [5, 33, 38][:u])), (100, ([0, 31, 32][:u], [64, 65, 99][:u]))):
            for at in places:
                P = T[cut:cut + m].copy()
                P[at] = ord("N")
                assert psearch(P, pt)[0] == 0
                for k in (u - 1, u, u + 2):
                    pos, dist = check(P, T, pt, k, what=(u, m, at, k))
                    if k == u - 1:
                        assert len(pos) == 0
                    else:
                        i = np.flatnonzero(pos == cut)
                        assert len(i) == 1 and dist[i[0]] == u and dist.min() >= u, (u, m, at, k)


@pytest.mark.parametrize("m", [1, 3, 7])
def test_k_at_least_m(m):
    n = 5003
    T = random_text(ACGT, n, 7200 + m)
    P = T[100:100 + m].copy()
    with PackedText.upload(T) as pt:
        pos, dist = check(P, T, pt, 7, what=m)
        assert len(pos) == n - m + 1 and np.array_equal(pos, np.arange(n - m + 1, dtype=np.uint64))
        assert dist.max() <= m and dist[100] == 0


def test_host_decisions():
    L = smart_amd.lib()
    T = random_text(ACGT, 5000, 7000)
    P = T[10:14].copy()
    with PackedText.upload(T) as pt:
        wpos, wdist = by_definition(P, T, 1)
        assert len(wpos) > 10
        # cap smaller than the count: SMARTGPU_ERR_NOMEM with count filled; cap = 0 with no buffer is a count
        out = np.zeros(4, dtype=np.uint64)
        mis = np.zeros(4, dtype=np.uint8)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_mis64(P.ctypes.data, 4, 1, pt._h, 0, len(T), out.ctypes.data, mis.ctypes.data, 4, ctypes.byref(c)) == -5
        assert c.value == len(wpos)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_mis64(P.ctypes.data, 4, 1, pt._h, 0, len(T), None, None, 0, ctypes.byref(c)) == -5
        assert c.value == len(wpos)
        # mismatches NULL with positions given
        out = np.zeros(len(wpos), dtype=np.uint64)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_mis64(P.ctypes.data, 4, 1, pt._h, 0, len(T), out.ctypes.data, None, len(out), ctypes.byref(c)) == 0
        assert c.value == len(wpos) and np.array_equal(out, wpos)
        assert pfind_mis(P, pt, 1, cap=4) == (None, None, len(wpos))
        assert pfind_mis(P, pt, 1, cap=0) == (None, None, len(wpos))
        # nothing within the budget: a count of 0 needs no room
        never = np.full(12, ord("N"), dtype=np.uint8)
        c = ctypes.c_uint64(9)
        assert L.smartgpu_pfind_mis64(never.ctypes.data, 12, 7, pt._h, 0, len(T), None, None, 0, ctypes.byref(c)) == 0 and c.value == 0
        with pytest.raises(smart_amd.SmartGpuError):
            psearch_mis(P, pt, 8)
        with pytest.raises(smart_amd.SmartGpuError):
            pfind_mis(P, pt, 1, off=4000, n=2000)  # a range outside the text
