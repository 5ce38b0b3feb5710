"""Packed texts on the GPU: planes_pack round trips and planes_scan counts against the count by definition
(oracle.search("bf", ...), the restatement of bf.c:25-39) and, at size, against the byte text's Shift-Or path.
Every count is exact; texts are built in numpy or by the counter-based generator."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import PackedText, Text, psearch, psearch_batch  # noqa: E402

VALUE_SETS = [(0, 1), (0, 255), (65, 67, 71, 84), (65, 67, 84), (7,)]
MS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 1000, 4200]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


class _ctx:
    """`with` for a Text (which has free() but is no context manager)."""

    def __init__(self, obj):
        self.obj = obj

    def __enter__(self):
        return self.obj

    def __exit__(self, *exc):
        self.obj.free()


def random_text(vals, n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]


def bf(oracle, P, T):
    """The count by definition; large products n * m (periodic and one-value texts) on several threads — the
    partition of the start positions is still the definition."""
    return oracle.search("bf", P, T, threads=16 if len(P) * len(T) > (1 << 26) else 1)


@pytest.mark.parametrize("vals", VALUE_SETS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4095, 4097, 2**20 + 3])
def test_round_trip(vals, n):
    T = random_text(vals, n, 1000 + n)
    present = sorted(set(T.tolist()))
    with _ctx(Text.upload(T)) as text:
        pt = PackedText.pack(text)
        try:
            assert len(pt) == n
            assert pt.symbols() == present
            planes, plane_bytes = smart_amd.ptext_layout(n, len(present))
            assert pt.planes == planes
            assert pt.nbytes == plane_bytes * planes
            assert np.array_equal(pt.read(0, n), T)
            for off, ln in ((0, 1), (n - 1, 1), (n // 2, n - n // 2), (n // 3, min(40, n - n // 3)), (min(31, n - 1), 1), (n, 0)):
                assert np.array_equal(pt.read(off, ln), T[off:off + ln]), (off, ln)
            assert np.array_equal(text.read(0, n), T)  # the byte text stays valid and independent
        finally:
            pt.free()
    with PackedText.upload(T) as pu:
        assert np.array_equal(pu.read(0, n), T)


@pytest.mark.parametrize("vals", VALUE_SETS)
@pytest.mark.parametrize("n", [33, 1000, 4097, 2**20 + 3])
def test_parity_grid(oracle, vals, n):
    T = random_text(vals, n, 2000 + n)
    checked = 0
    with PackedText.upload(T) as pt:
        for m in MS:
            if m > n:
                continue
            mid = (n - m) // 2
            pats = [T[0:m], T[n - m:n], T[mid:mid + m]]
            if len(vals) > 1:  # the middle one with one byte changed to another value of the text
                P = T[mid:mid + m].copy()
                j = m // 2
                P[j] = next(v for v in vals if v != P[j])
                pats.append(P)
            for P in pats:
                got = psearch(P, pt)[0]
                want = bf(oracle, P, T)
                print("vals=%s n=%d m=%d got=%d want=%d" % (vals, n, m, got, want))
                assert got == want, (vals, n, m)
                checked += 1
    assert checked >= 3


@pytest.mark.parametrize("unit_len", [1, 2, 3, 4, 5, 6, 7])
def test_periodic_texts(oracle, unit_len):
    n = 2**16 + 5
    for vals in ((0, 1), (65, 67, 71, 84)):
        rng = np.random.default_rng(3000 + unit_len + len(vals))
        unit = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), unit_len)]
        T = np.resize(unit, n)
        with PackedText.upload(T) as pt:
            for m in (1, 2, 7, 8, 31, 32, 33, 64, 100, 1000, 4200):
                for k in (0, 1, unit_len - 1):
                    P = T[k:k + m]
                    got = psearch(P, pt)[0]
                    want = bf(oracle, P, T)
                    print("unit=%s m=%d k=%d got=%d want=%d" % (unit.tolist(), m, k, got, want))
                    assert got == want, (unit.tolist(), m, k)
                    if len(set(unit.tolist())) == 1:
                        assert got == n - m + 1


def test_one_value_text_counts_every_window():
    n = 2**20 + 3
    T = np.full(n, 7, dtype=np.uint8)
    with PackedText.upload(T) as pt:
        for m in (1, 31, 32, 33, 4200):
            assert psearch(T[:m], pt)[0] == n - m + 1, m


@pytest.mark.parametrize("vals", [(0, 1), (65, 67, 71, 84), (3, 200, 255)])
@pytest.mark.parametrize("n", [1000 + 13, 4097, 33, 95])
def test_the_pad_is_not_text(oracle, vals, n):
    """The zero pad behind (and before) the planes looks like code 0.  A text that ends in code-0 symbols and a pattern of m
    code-0 symbols: only windows inside the text count; the same at the front of a range that starts at off > 0."""
    assert n % 32 != 0
    T = random_text(vals, n, 4000 + n)
    zero = min(vals)  # code 0
    tail = min(n // 2, 300)
    T[n - tail:] = zero
    T[:tail] = zero
    with PackedText.upload(T) as pt:
        for m in (1, 2, 5, 31, 32, 33, 64, 100, 257):
            if m > tail:
                continue
            P = np.full(m, zero, dtype=np.uint8)
            want = bf(oracle, P, T)
            got = psearch(P, pt)[0]
            print("n=%d m=%d got=%d want=%d" % (n, m, got, want))
            assert got == want, (n, m)
            for off in (1, 5, 31, 32, 33):
                if off + m > n:
                    continue
                want = bf(oracle, P, T[off:])
                assert psearch(P, pt, off=off)[0] == want, (n, m, off)
                ln = min(n - off, tail + 3)
                assert psearch(P, pt, off=off, n=ln)[0] == bf(oracle, P, T[off:off + ln]), (n, m, off, ln)


@pytest.mark.parametrize("vals", [(0, 1), (65, 67, 71, 84)])
def test_sub_ranges(oracle, vals):
    n = 20000
    T = random_text(vals, n, 5000)
    T[5000:5600] = vals[0]  # a run, so that short patterns of it occur densely across dword borders
    with PackedText.upload(T) as pt:
        for m in (1, 3, 32, 40):
            for P in (T[5100:5100 + m], T[777:777 + m]):
                for off in (0, 1, 31, 32, 4992, 5000, 5023):
                    for end_word_off in (0, 1, 31):
                        for words in (0, 1, 3, 17, 150):
                            end = (off // 32 + words) * 32 + end_word_off
                            if end < off or end > n:
                                continue
                            ln = end - off
                            want = bf(oracle, P, T[off:off + ln])
                            got = psearch(P, pt, off=off, n=ln)[0]
                            assert got == want, (vals, m, off, ln, got, want)


def test_refusals(oracle):
    T5 = np.resize(np.array([1, 2, 3, 4, 5], dtype=np.uint8), 1000)
    with _ctx(Text.upload(T5)) as text:
        with pytest.raises(smart_amd.SmartGpuError, match="5"):
            PackedText.pack(text)
    with pytest.raises(smart_amd.SmartGpuError, match="5"):
        PackedText.upload(T5)
    T = random_text((65, 67, 71, 84), 5000, 6000)
    with PackedText.upload(T) as pt:
        assert psearch(np.array([65, 66, 67], dtype=np.uint8), pt)[0] == 0       # 66: a byte the text does not hold
        assert psearch(np.full(40, 0, dtype=np.uint8), pt)[0] == 0
        for bad in (np.zeros(0, dtype=np.uint8), np.full(4201, 65, dtype=np.uint8)):
            rc = smart_amd.lib().smartgpu_psearch64(bad.ctypes.data, len(bad), pt._h, 0, len(pt), None, None, None)
            assert rc == -3, (len(bad), rc)  # SMARTGPU_ERR_ARG
            with pytest.raises(smart_amd.SmartGpuError):
                psearch(bad, pt)
        assert psearch(T[:100], pt, off=10, n=50)[0] == 0   # m > n
        with pytest.raises(smart_amd.SmartGpuError):
            psearch(T[:4], pt, off=4000, n=2000)            # range outside the text
    short = random_text((0, 1), 20, 6001)
    with PackedText.upload(short) as pt:
        assert psearch(np.zeros(21, dtype=np.uint8), pt)[0] == 0  # m > n


def test_batch_equals_single_calls(oracle):
    T = random_text((65, 67, 71, 84), 300000, 7000)
    rng = np.random.default_rng(7001)
    with PackedText.upload(T) as pt:
        for m in (6, 40):
            pats = []
            for i in range(64):
                k = int(rng.integers(0, len(T) - m))
                P = T[k:k + m].copy()
                if i % 3 == 1:
                    P[m // 2] = 66  # a miss: not a symbol of the text
                if i % 3 == 2:
                    P = np.asarray((65, 67, 71, 84), dtype=np.uint8)[rng.integers(0, 4, m)]  # hit or miss
                pats.append(P)
            counts, batch_ms = psearch_batch(pats, pt)
            singles = [psearch(P, pt)[0] for P in pats]
            assert counts.tolist() == singles
            assert counts.tolist() == [bf(oracle, P, T) for P in pats]
            assert any(c > 0 for c in singles) and any(c == 0 for c in singles)
            sub, _ = psearch_batch(pats, pt, off=1001, n=77777)
            assert sub.tolist() == [psearch(P, pt, off=1001, n=77777)[0] for P in pats]


@pytest.mark.parametrize("sigma", [4, 2])
def test_against_the_byte_text_at_size(oracle, sigma):
    n = 1 << 30
    text = Text.generate(0x5EED0300 + sigma, sigma, n)
    try:
        with PackedText.pack(text) as pt:
            assert pt.planes == (2 if sigma == 4 else 1) and pt.nbytes == pt.planes * (n // 8)
            for m in (4, 8, 32, 256, 4096):
                for k in (0, 123456789, n // 2 + 31, n - m):
                    P = text.read(k, m)
                    got = psearch(P, pt)[0]
                    want = smart_amd.search("so", P, text)[0]
                    print("sigma=%d m=%d k=%d got=%d want=%d" % (sigma, m, k, got, want))
                    assert got == want and got >= 1, (sigma, m, k)
            off, ln = 777 * (1 << 20) + 13, 8 << 20
            S = text.read(off, ln)
            assert np.array_equal(pt.read(off, ln), S)
            for m in (4, 8, 32):
                P = S[5000:5000 + m]
                assert psearch(P, pt, off=off, n=ln)[0] == bf(oracle, P, S), m
    finally:
        text.free()


def test_beyond_2_to_the_32_positions(oracle):
    n = 8 << 30
    text = Text.generate(0x5EED0308, 4, n)
    try:
        with PackedText.pack(text) as pt:
            assert len(pt) == n and pt.planes == 2 and pt.nbytes == n // 4
            P = text.read((1 << 32) + 5, 16)
            got = psearch(P, pt)[0]
            want = smart_amd.search("so", P, text)[0]
            print("8 GiB m=16 got=%d want=%d" % (got, want))
            assert got == want and got >= 1
            for off in ((1 << 32) - (1 << 19), n - (1 << 20)):
                S = text.read(off, 1 << 20)
                assert np.array_equal(pt.read(off, 1 << 20), S)
                for m in (3, 9, 16, 40):
                    Q = S[(1 << 19) - 4:(1 << 19) - 4 + m]
                    assert psearch(Q, pt, off=off, n=1 << 20)[0] == bf(oracle, Q, S), (off, m)
    finally:
        text.free()


FUZZ_CASES = 20000


def test_differential_fuzz(oracle):
    """20,000 random (value set, n <= 65,536, m, kind, off, len) cases from one seed against the count by definition."""
    rng = np.random.default_rng(0x9A7E5)
    ran = 0
    for case in range(FUZZ_CASES):
        k = int(rng.integers(1, 5))
        vals = np.sort(rng.choice(256, size=k, replace=False)).astype(np.uint8)
        n = int(2 ** rng.uniform(0, 16)) if case % 4 else int(rng.integers(1, 65537))
        n = max(1, min(n, 65536))
        kind = ("random", "periodic", "mutated")[int(rng.integers(0, 3))]
        if kind == "periodic":
            unit = vals[rng.integers(0, k, int(rng.integers(1, 40)))]
            T = np.resize(unit, n)
        else:
            T = vals[rng.integers(0, k, n)]
        off = int(rng.integers(0, n))
        ln = int(rng.integers(1, n - off + 1))
        if rng.integers(0, 4) == 0:
            off, ln = 0, n
        m = max(1, min(int(2 ** rng.uniform(0, 12.1)), 4200, ln + (1 if rng.integers(0, 50) == 0 else 0)))
        if m <= n:
            s = int(rng.integers(0, n - m + 1))
            P = T[s:s + m].copy()
        else:
            P = vals[rng.integers(0, k, m)]
        if kind == "mutated" and k > 1:
            j = int(rng.integers(0, m))
            P[j] = vals[(int(np.searchsorted(vals, P[j])) + 1) % k]
        with PackedText.upload(T) as pt:
            got = psearch(P, pt, off=off, n=ln)[0]
        want = bf(oracle, P, T[off:off + ln])
        assert got == want, dict(case=case, vals=vals.tolist(), n=n, kind=kind, off=off, len=ln, m=m, got=got, want=want)
        ran += 1
        if ran % 2000 == 0:
            print("fuzz: %d cases" % ran, flush=True)
    assert ran == FUZZ_CASES
