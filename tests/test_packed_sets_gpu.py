"""Set patterns on packed texts on the GPU (planes_sets_scan, planes_sets_find): counts and positions against the DEFINITION,
computed here with numpy — start position s survives when, for every j < m, the code of T[s + j] is a member of sets[j].
Every comparison is exact equality; no text is longer than 2^20 + 3 symbols."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import PackedText, pfind, pfind_sets, psearch, psearch_sets  # noqa: E402

from test_packed_text_gpu import MS, VALUE_SETS  # noqa: E402

ACGT = (65, 67, 71, 84)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def random_text(vals, n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]


def by_definition(sets, T, symbols, off=0, n=None):
    """The ascending start positions (relative to symbol 0) in [off, off + n - m] by the definition, as uint64."""
    n = len(T) - off if n is None else n
    m = len(sets)
    if m > n:
        return np.zeros(0, dtype=np.uint64)
    s = np.arange(off, off + n - m + 1, dtype=np.int64)
    tables = {}
    for j in range(m):
        accept = tables.get(int(sets[j]))  # accept[j]: the byte values position j takes
        if accept is None:
            accept = np.zeros(256, dtype=bool)
            for c, v in enumerate(symbols):
                accept[v] = bool(int(sets[j]) >> c & 1)
            tables[int(sets[j])] = accept
        if accept[list(symbols)].all():
            continue  # every value T holds (symbols: pt.symbols()) is accepted: the gather would keep all of s
        s = s[accept[T[s + j]]]
        if len(s) == 0:
            break
    return s.astype(np.uint64)


def check(sets, T, pt, symbols, off=0, n=None, what=None):
    """Count and positions of both calls against the definition; returns the count."""
    sets = np.asarray(sets, dtype=np.uint8)
    want = by_definition(sets, T, symbols, off, n)
    got = psearch_sets(sets, pt, off=off, n=n)[0]
    assert got == len(want), (what, got, len(want))
    pos, cnt = pfind_sets(sets, pt, off=off, n=n, cap=max(len(want), 1))
    assert cnt == len(want) and pos is not None and pos.dtype == np.uint64, (what, cnt, len(want))
    assert np.array_equal(pos, want), what
    return len(want)


def singletons(P, symbols):
    code = {v: c for c, v in enumerate(symbols)}
    return np.asarray([1 << code[int(b)] for b in P], dtype=np.uint8)


@pytest.mark.parametrize("vals", [ACGT, (0, 255)])
def test_every_table_at_every_position(vals):
    """m = 40 full sets with position j set to s: every case of the kernels' switch at each of the first 32 positions,
    and planes_sets_verify for j >= 32."""
    n, m = 4097, 40
    T = random_text(vals, n, 100 + len(vals))
    full = (1 << len(vals)) - 1
    with PackedText.upload(T) as pt:
        sym = pt.symbols()
        assert sym == list(vals)
        for s in range(1, full + 1):
            for j in range(m):
                sets = np.full(m, full, dtype=np.uint8)
                sets[j] = s
                check(sets, T, pt, sym, what=(vals, s, j))


@pytest.mark.parametrize("vals", VALUE_SETS)
@pytest.mark.parametrize("n", [33, 4097, 2**20 + 3])
def test_singleton_sets_equal_the_exact_matcher(vals, n):
    T = random_text(vals, n, 2000 + n)
    checked = 0
    with PackedText.upload(T) as pt:
        sym = pt.symbols()
        for m in MS:
            if m > n:
                continue
            mid = (n - m) // 2
            pats = [T[mid:mid + m]]
            if len(vals) > 1:  # the same with one symbol changed to another value of the text
                P = T[mid:mid + m].copy()
                P[m // 2] = next(v for v in vals if v != P[m // 2])
                pats.append(P)
            for P in pats:
                sets = singletons(P, sym)
                want = psearch(P, pt)[0]
                assert psearch_sets(sets, pt)[0] == want, (vals, n, m)
                wpos, wcnt = pfind(P, pt, cap=max(want, 1))
                gpos, gcnt = pfind_sets(sets, pt, cap=max(want, 1))
                assert gcnt == wcnt == want and np.array_equal(gpos, wpos), (vals, n, m)
                checked += 1
    assert checked >= 2


RANDOM_MS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 1000, 4200]


def random_sets(rng, window, sym, two_member_prefix=0):
    """Per position: a singleton (of the text's window, so some patterns occur) with probability 0.7, a two- or three-member
    set (holding the window's symbol) with 0.2, the full set with 0.1; the first `two_member_prefix` positions all two-member."""
    k = len(sym)
    full = (1 << k) - 1
    base = singletons(window, sym)
    sets = base.copy()
    for j in range(len(sets)):
        r = rng.random()
        if j < two_member_prefix or 0.7 <= r < 0.9:
            size = 2 if j < two_member_prefix else int(rng.integers(2, 4))
            size = min(size, k)
            others = [c for c in range(k) if not (int(base[j]) >> c & 1)]
            extra = rng.choice(others, size=size - 1, replace=False) if size > 1 else []
            for c in extra:
                sets[j] |= 1 << int(c)
        elif r >= 0.9:
            sets[j] = full
    return sets


@pytest.mark.parametrize("vals", [ACGT, (0, 255), (65, 67, 84)])
@pytest.mark.parametrize("n", [1000, 2**16 + 5, 2**20 + 3])
def test_random_sets(vals, n):
    T = random_text(vals, n, 3000 + n + len(vals))
    rng = np.random.default_rng(3100 + n + len(vals))
    total = 0
    with PackedText.upload(T) as pt:
        sym = pt.symbols()
        for m in RANDOM_MS:
            if m > n:
                continue
            for prefix in (0, 8, 32):  # two-member sets at the first 8 / 32 positions: the wave does not leave early
                k = int(rng.integers(0, n - m + 1))
                sets = random_sets(rng, T[k:k + m], sym, two_member_prefix=min(prefix, m))
                total += check(sets, T, pt, sym, what=(vals, n, m, prefix))
    assert total > 0


@pytest.mark.parametrize("unit_len", [1, 2, 3, 4, 5, 6, 7])
def test_periodic_and_one_value_texts(unit_len):
    """Sets that contain the unit's symbols: many survivors per lane reach planes_sets_verify, the output stage is dense."""
    n = 2**16 + 5
    for vals in ((0, 1), ACGT):
        rng = np.random.default_rng(4000 + unit_len + len(vals))
        unit = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), unit_len)]
        T = np.resize(unit, n)
        with PackedText.upload(T) as pt:
            sym = pt.symbols()
            k = len(sym)
            present = sum(1 << c for c in range(k))  # every symbol the text holds
            for m in (8, 33, 100, 4200):
                base = singletons(T[1:1 + m], sym)
                widened = base.copy()
                widened[::3] = present  # every third position accepts all of the unit's symbols
                for sets in (base, widened):
                    check(sets, T, pt, sym, what=(unit.tolist(), m))
                fullsets = np.full(m, present, dtype=np.uint8)
                assert psearch_sets(fullsets, pt)[0] == n - m + 1
                pos, cnt = pfind_sets(fullsets, pt, cap=n)
                assert cnt == n - m + 1 and np.array_equal(pos, np.arange(n - m + 1, dtype=np.uint64))
                if k > 1 and m <= 100:  # all but one position full: the kernels run, nearly every position survives
                    almost = fullsets.copy()
                    almost[m - 1] = int(base[m - 1])
                    check(almost, T, pt, sym, what=(unit.tolist(), m, "almost full"))


@pytest.mark.parametrize("vals", [(0, 1), ACGT, (3, 200, 255)])
@pytest.mark.parametrize("n", [1000 + 13, 4097, 33, 95])
def test_the_pad_is_not_text(vals, n):
    """The zero pad around the planes looks like code 0: a text that begins and ends in code-0 symbols, sets that contain
    code 0 — only windows inside the text count."""
    assert n % 32 != 0
    T = random_text(vals, n, 5000 + n)
    tail = min(n // 2, 300)
    T[n - tail:] = min(vals)
    T[:tail] = min(vals)
    T[tail] = vals[1]  # between the two runs (n = 33 leaves one symbol there): the text holds code 1, so {code 0, code 1} is a set of it
    with PackedText.upload(T) as pt:
        sym = pt.symbols()
        assert len(sym) >= 2
        for m in (1, 2, 5, 31, 32, 33, 64, 100, 257):
            if m > tail:
                continue
            for s in (1, 3):  # {code 0}, {code 0, code 1}
                sets = np.full(m, s, dtype=np.uint8)
                check(sets, T, pt, sym, what=(n, m, s))
                for off in (1, 31, 32, 33):
                    if off + m > n:
                        continue
                    check(sets, T, pt, sym, off=off, what=(n, m, s, off))
                    check(sets, T, pt, sym, off=off, n=min(n - off, tail + 3), what=(n, m, s, off, "short"))


def test_sub_ranges():
    n = 2**17 + 77
    T = random_text(ACGT, n, 6000)
    T[60000:70000] = 65  # a run across 65536: dense survivors around the borders
    with PackedText.upload(T) as pt:
        sym = pt.symbols()
        for m in (1, 3, 32, 40):
            sets = np.full(m, 1 | 4, dtype=np.uint8)  # A or G
            sets[0] = 1
            edges = sorted({b + d for b in (0, 32, 128, 8192, 65536) for d in (-1, 0, 1) if b + d >= 0})
            for off in edges:
                for end in edges + [n]:
                    if end < off:
                        continue
                    check(sets, T, pt, sym, off=off, n=end - off, what=(m, off, end))
        assert psearch_sets(np.full(100, 15, dtype=np.uint8), pt, off=10, n=50)[0] == 0  # m > n
        pos, cnt = pfind_sets(np.full(100, 1, dtype=np.uint8), pt, off=10, n=50)
        assert cnt == 0 and len(pos) == 0


def test_host_decisions():
    L = smart_amd.lib()
    import ctypes
    T = random_text(ACGT, 5000, 7000)
    with PackedText.upload(T) as pt:
        sets = np.full(40, 15, dtype=np.uint8)
        sets[17] = 0  # an empty set: nothing matches
        assert psearch_sets(sets, pt)[0] == 0
        pos, cnt = pfind_sets(sets, pt)
        assert cnt == 0 and len(pos) == 0
        with pytest.raises(smart_amd.SmartGpuError, match="position 5"):
            bad = np.full(8, 1, dtype=np.uint8)
            bad[5] = 16  # bits 4..7 are never codes
            psearch_sets(bad, pt)
        with pytest.raises(smart_amd.SmartGpuError):
            psearch_sets(np.full(4, 1, dtype=np.uint8), pt, off=4000, n=2000)  # a range outside the text
        with pytest.raises(smart_amd.SmartGpuError):
            pfind_sets(np.full(4, 1, dtype=np.uint8), pt, off=5001, n=0)
        # cap smaller than the count: SMARTGPU_ERR_NOMEM with count filled; cap = 0 with no buffer is a count
        one = np.asarray([1, 1 | 2], dtype=np.uint8)
        want = by_definition(one, T, pt.symbols())
        assert len(want) > 10
        out = np.zeros(4, dtype=np.uint64)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_sets64(one.ctypes.data, 2, pt._h, 0, len(T), out.ctypes.data, 4, ctypes.byref(c)) == -5
        assert c.value == len(want)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_pfind_sets64(one.ctypes.data, 2, pt._h, 0, len(T), None, 0, ctypes.byref(c)) == -5
        assert c.value == len(want)
        assert pfind_sets(one, pt, cap=4) == (None, len(want))
        assert pfind_sets(one, pt, cap=0) == (None, len(want))
        never = np.full(3, 1, dtype=np.uint8)
        never[1] = 0
        c = ctypes.c_uint64(9)
        assert L.smartgpu_pfind_sets64(never.ctypes.data, 3, pt._h, 0, len(T), None, 0, ctypes.byref(c)) == 0 and c.value == 0
        # full sets with too little room: the count all the same
        assert pfind_sets(np.full(3, 15, dtype=np.uint8), pt, cap=10) == (None, len(T) - 2)
    with PackedText.upload(random_text((65, 67, 84), 3000, 7001)) as pt3:
        with pytest.raises(smart_amd.SmartGpuError, match="position 2"):
            psearch_sets(np.asarray([1, 2, 8, 4], dtype=np.uint8), pt3)
        with pytest.raises(smart_amd.SmartGpuError, match="position 2"):
            pfind_sets(np.asarray([1, 2, 8, 4], dtype=np.uint8), pt3)
    with PackedText.upload(random_text((0, 255), 3000, 7002)) as pt2:
        with pytest.raises(smart_amd.SmartGpuError, match="position 1"):
            psearch_sets(np.asarray([1, 4, 2], dtype=np.uint8), pt2)
        with pytest.raises(smart_amd.SmartGpuError, match="position 1"):
            pfind_sets(np.asarray([1, 4, 2], dtype=np.uint8), pt2)


def test_iupac_end_to_end():
    rng = np.random.default_rng(8000)
    T = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 100003)].copy()
    planted = {b"GGATCC": (17, 4095, 8190, 65533, 99990), b"GGTACC": (31, 40000), b"GGCGCC": (64, 77777)}
    for site, where in planted.items():
        for p in where:
            T[p:p + 6] = np.frombuffer(site, dtype=np.uint8)
    with PackedText.upload(T) as pt:
        sym = pt.symbols()
        for motif in (b"GGNNCC", b"GGWWCC", b"ggatcc", b"GGSSCC"):
            sets = pt.iupac(motif)
            assert np.array_equal(sets, smart_amd.iupac_sets(motif, sym))
            count = check(sets, T, pt, sym, what=motif)
            assert count >= 2
        found = set(pfind_sets(pt.iupac(b"GGNNCC"), pt)[0].tolist())
        assert all(p in found for where in planted.values() for p in where)
        ww = set(pfind_sets(pt.iupac(b"GGWWCC"), pt)[0].tolist())
        assert all(p in ww for p in planted[b"GGATCC"] + planted[b"GGTACC"]) and not any(p in ww for p in planted[b"GGCGCC"])


def test_the_byte_text_is_not_needed():
    T = random_text(ACGT, 70001, 9000)
    with PackedText.upload(T) as pt:  # the byte copy is released by upload
        check(pt.iupac(b"TATAWAW"), T, pt, pt.symbols(), what="TATAWAW")
        assert np.array_equal(pt.read(0, len(T)), T)
