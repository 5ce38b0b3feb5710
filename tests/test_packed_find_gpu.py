"""Positions on packed texts on the GPU: pfind / pfind_batch (planes_find) against the positions BY DEFINITION, computed in
numpy by positions_by_definition() below — candidates T[s] == P[0], refined symbol by symbol — which shares nothing with the
code under test; at size against smart_amd.find on the byte text of the same symbols.  Every comparison is np.array_equal on
uint64 arrays plus count == len(want) == psearch's count."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import PackedText, Text, pfind, pfind_batch, psearch, psearch_batch  # noqa: E402

VALUE_SETS = [(0, 1), (0, 255), (65, 67, 71, 84), (65, 67, 84), (7,)]
MS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 1000, 4200]
OK, ERR_ARG, ERR_NOMEM = 0, -3, -5


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def random_text(vals, n, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), n)]


def positions_by_definition(P, T, off=0, ln=None):
    """Every s in [off, off+ln-m] with T[s+j] == P[j] for all j < m, ascending, relative to T[0], as uint64.
    While most start positions are alive they are kept as a mask (whole-array compares), then as a list of candidates."""
    P = np.asarray(P, dtype=np.uint8)
    if ln is None:
        ln = len(T) - off
    m = len(P)
    if m > ln:
        return np.zeros(0, dtype=np.uint64)
    S = T[off:off + ln]
    L = ln - m + 1
    alive = S[:L] == P[0]
    j = 1
    while j < m and 8 * int(np.count_nonzero(alive)) > L:
        alive &= S[j:j + L] == P[j]
        j += 1
    cand = np.flatnonzero(alive)
    while j < m and cand.size:
        cand = cand[S[cand + j] == P[j]]
        j += 1
    return (cand + off).astype(np.uint64)


def check(P, pt, want, off=0, ln=None, slack=3):
    """One comparison: pfind's list and count against `want`, and the count against psearch."""
    got, count = pfind(P, pt, off=off, n=ln, cap=len(want) + slack)
    assert got is not None, (len(P), off, ln, count, len(want))
    assert got.dtype == np.uint64 and want.dtype == np.uint64
    assert np.array_equal(got, want), (len(P), off, ln, count, len(want), got[:8], want[:8])
    assert count == len(want) == psearch(P, pt, off=off, n=ln)[0], (len(P), off, ln, count, len(want))
    return 1


def pfind_c(P, pt, off, ln, cap, guard=0):
    """smartgpu_pfind64 itself: (rc, count, the buffer of cap + guard entries pre-filled with a guard value)."""
    P = np.ascontiguousarray(P, dtype=np.uint8)
    fill = np.uint64(0xDEADBEEFDEADBEEF)
    buf = np.full(cap + guard, fill, dtype=np.uint64)
    c = ctypes.c_uint64(0xFFFFFFFF)
    rc = smart_amd.lib().smartgpu_pfind64(P.ctypes.data, len(P), pt._h, off, ln, buf.ctypes.data if cap else None, cap, ctypes.byref(c))
    return rc, int(c.value), buf


@pytest.mark.parametrize("vals", VALUE_SETS)
@pytest.mark.parametrize("n", [33, 1000, 4097, 2**20 + 3])
def test_grid(vals, n):
    T = random_text(vals, n, 2000 + n)
    checked = 0
    with PackedText.upload(T) as pt:
        for m in MS:
            if m > n:
                continue
            mid = (n - m) // 2
            pats = [T[0:m], T[n - m:n], T[mid:mid + m]]
            if len(vals) > 1:  # the middle one with one symbol changed to another value of the text
                P = T[mid:mid + m].copy()
                j = m // 2
                P[j] = next(v for v in vals if v != P[j])
                pats.append(P)
            for P in pats:
                checked += check(P, pt, positions_by_definition(P, T))
    assert checked == sum((4 if len(vals) > 1 else 3) for m in MS if m <= n)


@pytest.mark.parametrize("vals", [(0, 1), (65, 67, 71, 84)])
def test_sub_ranges(vals):
    """Positions stay relative to symbol 0, and only windows inside [off, off+n) are reported."""
    n = 20000
    T = random_text(vals, n, 5000)
    T[5000:5600] = vals[0]  # a run, so that short patterns of it occur densely across dword borders
    checked = expected = 0
    with PackedText.upload(T) as pt:
        for m in (1, 3, 32, 40):
            for P in (T[5100:5100 + m], T[777:777 + m]):
                for off in (0, 1, 31, 32, 4992, 5000, 5023):
                    for end_word_off in (0, 1, 31):
                        for words in (0, 1, 3, 17, 150):
                            end = (off // 32 + words) * 32 + end_word_off
                            if end < off or end > n:
                                continue
                            expected += 1
                            ln = end - off
                            want = positions_by_definition(P, T, off, ln)
                            assert want.size == 0 or (int(want[0]) >= off and int(want[-1]) + m <= off + ln)
                            checked += check(P, pt, want, off=off, ln=ln)
    assert checked == expected and checked > 700


@pytest.mark.parametrize("vals", [(0, 1), (65, 67, 71, 84), (3, 200, 255)])
@pytest.mark.parametrize("n", [1000 + 13, 4097, 33, 95])
def test_the_pad_is_not_text(vals, n):
    """The zero pad behind (and before) the planes looks like code 0: a text that begins and ends in code-0 symbols, patterns
    of m code-0 symbols, n % 32 != 0 — only windows inside the text and the range are positions."""
    assert n % 32 != 0
    T = random_text(vals, n, 4000 + n)
    zero = min(vals)  # code 0
    tail = min(n // 2, 300)
    T[n - tail:] = zero
    T[:tail] = zero
    checked = expected = 0
    with PackedText.upload(T) as pt:
        for m in (1, 2, 5, 31, 32, 33, 64, 100, 257):
            if m > tail:
                continue
            P = np.full(m, zero, dtype=np.uint8)
            want = positions_by_definition(P, T)
            assert int(want[-1]) == n - m
            expected += 1
            checked += check(P, pt, want)
            for off in (1, 5, 31, 32, 33):
                if off + m > n:
                    continue
                expected += 2
                checked += check(P, pt, positions_by_definition(P, T, off), off=off)
                ln = min(n - off, tail + 3)
                checked += check(P, pt, positions_by_definition(P, T, off, ln), off=off, ln=ln)
    assert checked == expected and checked >= 1


def test_dense_one_value_text():
    n = 2**20 + 3
    T = np.full(n, 7, dtype=np.uint8)
    checked = 0
    with PackedText.upload(T) as pt:
        for m in (1, 31, 32, 33, 4200):
            checked += check(T[:m], pt, np.arange(n - m + 1, dtype=np.uint64))
        assert np.array_equal(positions_by_definition(T[:33], T), np.arange(n - 32, dtype=np.uint64))  # the definition agrees
    assert checked == 5


@pytest.mark.parametrize("unit_len", [1, 2, 3, 4, 5, 6, 7])
def test_dense_periodic_texts(unit_len):
    """Long patterns on periodic texts: planes_verify with many survivors per lane, then the output stage."""
    n = 2**16 + 5
    checked = 0
    for vals in ((0, 1), (65, 67, 71, 84)):
        rng = np.random.default_rng(3000 + unit_len + len(vals))
        unit = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), unit_len)]
        T = np.resize(unit, n)
        with PackedText.upload(T) as pt:
            for m in (1, 2, 7, 8, 31, 32, 33, 64, 100, 1000, 4200):
                for k in (0, 1, unit_len - 1):
                    P = T[k:k + m]
                    want = positions_by_definition(P, T)
                    assert len(want) >= (n - m + 1) // unit_len
                    checked += check(P, pt, want)
    assert checked == 2 * 11 * 3


def test_capacity():
    T = random_text((65, 67, 71, 84), 300000, 8000)
    with PackedText.upload(T) as pt:
        for m in (2, 5, 40):
            P = T[1234:1234 + m]
            want = positions_by_definition(P, T)
            count = len(want)
            assert count >= 1
            # cap = count - 1: no list, the count is right
            got, c = pfind(P, pt, cap=count - 1)
            assert got is None and c == count
            rc, c, buf = pfind_c(P, pt, 0, len(T), count - 1, guard=4)
            assert rc == ERR_NOMEM and c == count
            msg = smart_amd.lib().smartgpu_last_error().decode()
            assert str(count) in msg and str(count - 1) in msg, msg
            assert np.all(buf[count - 1:] == np.uint64(0xDEADBEEFDEADBEEF))
            # cap = 0 and a NULL buffer: a count
            rc, c, _ = pfind_c(P, pt, 0, len(T), 0)
            assert (rc, c) == (OK if count == 0 else ERR_NOMEM, count)
            got, c = pfind(P, pt, cap=0)
            assert got is None and c == count
            # cap = count exactly: the full list, and nothing behind positions[cap] is touched
            rc, c, buf = pfind_c(P, pt, 0, len(T), count, guard=16)
            assert rc == OK and c == count
            assert np.array_equal(buf[:count], want)
            assert np.all(buf[count:] == np.uint64(0xDEADBEEFDEADBEEF))
            got, c = pfind(P, pt, cap=count)
            assert c == count and np.array_equal(got, want)
        # a byte the text does not hold, m > n: zero, OK, nothing written
        for P, off, ln in ((np.array([65, 66, 67], dtype=np.uint8), 0, len(T)), (T[:100], 10, 50)):
            rc, c, buf = pfind_c(P, pt, off, ln, 8, guard=2)
            assert (rc, c) == (OK, 0) and np.all(buf == np.uint64(0xDEADBEEFDEADBEEF))
            got, c = pfind(P, pt, off=off, n=ln)
            assert c == 0 and got.dtype == np.uint64 and len(got) == 0
        rc, c, _ = pfind_c(np.array([66], dtype=np.uint8), pt, 0, len(T), 0)
        assert (rc, c) == (OK, 0)  # cap = 0, no occurrence: complete


def test_refusals_with_a_handle():
    T = random_text((65, 67, 71, 84), 5000, 6000)
    L = smart_amd.lib()
    out = np.zeros(8, dtype=np.uint64)
    c = ctypes.c_uint64(0)
    with PackedText.upload(T) as pt:
        for bad in (np.zeros(0, dtype=np.uint8), np.full(4201, 65, dtype=np.uint8)):
            assert L.smartgpu_pfind64(bad.ctypes.data, len(bad), pt._h, 0, len(pt), out.ctypes.data, 8, ctypes.byref(c)) == ERR_ARG
            with pytest.raises(smart_amd.SmartGpuError):
                pfind(bad, pt)
        P = T[:4].copy()
        assert L.smartgpu_pfind64(P.ctypes.data, 4, pt._h, 0, len(pt), out.ctypes.data, 8, None) == ERR_ARG
        assert L.smartgpu_pfind64(P.ctypes.data, 4, pt._h, 0, len(pt), None, 8, ctypes.byref(c)) == ERR_ARG
        assert L.smartgpu_last_error().decode() != ""
        with pytest.raises(smart_amd.SmartGpuError):
            pfind(P, pt, off=4000, n=2000)  # range outside the text
        ptrs = (ctypes.c_void_p * 1)(P.ctypes.data)
        starts = np.zeros(2, dtype=np.uint64)
        assert L.smartgpu_pfind_batch64(ctypes.cast(ptrs, ctypes.c_void_p), 4, 0, pt._h, 0, len(pt), out.ctypes.data, 8, starts.ctypes.data) == ERR_ARG
        assert L.smartgpu_pfind_batch64(ctypes.cast(ptrs, ctypes.c_void_p), 4, 1, pt._h, 0, len(pt), out.ctypes.data, 8, None) == ERR_ARG
        assert L.smartgpu_pfind_batch64(ctypes.cast(ptrs, ctypes.c_void_p), 4, 1, pt._h, 0, len(pt), None, 8, starts.ctypes.data) == ERR_ARG


def test_batch_equals_single_calls():
    T = random_text((65, 67, 71, 84), 300000, 7000)
    rng = np.random.default_rng(7001)
    compared = 0
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
            for off, ln in ((0, len(T)), (1001, 77777)):
                lists, counts = pfind_batch(pats, pt, off=off, n=ln)
                ref_counts, _ = psearch_batch(pats, pt, off=off, n=ln)
                assert lists is not None and len(lists) == 64
                assert counts.dtype == np.uint64 and np.array_equal(counts, ref_counts)
                for P, got, c in zip(pats, lists, counts):
                    single, sc = pfind(P, pt, off=off, n=ln)
                    assert got.dtype == np.uint64 and np.array_equal(got, single) and sc == c == len(got)
                    assert np.array_equal(got, positions_by_definition(P, T, off, ln))
                    compared += 1
                assert any(c > 0 for c in counts) and any(c == 0 for c in counts)
                # starts itself, and too small a cap: starts is still complete, no list
                total = int(counts.sum())
                assert total >= 2
                ptrs = (ctypes.c_void_p * 64)(*[p.ctypes.data for p in pats])
                for cap in (total, total - 1, 0):
                    starts = np.full(65, 99, dtype=np.uint64)
                    buf = np.full(total + 4, np.uint64(0xDEADBEEFDEADBEEF), dtype=np.uint64)
                    rc = smart_amd.lib().smartgpu_pfind_batch64(ctypes.cast(ptrs, ctypes.c_void_p), m, 64, pt._h, off, ln,
                                                                buf.ctypes.data if cap else None, cap, starts.ctypes.data)
                    assert rc == (OK if cap >= total else ERR_NOMEM), (cap, total, rc)
                    assert np.array_equal(starts, np.concatenate(([0], np.cumsum(ref_counts))).astype(np.uint64))
                    assert np.all(buf[cap:] == np.uint64(0xDEADBEEFDEADBEEF))
                    if cap >= total:
                        assert np.array_equal(buf[:total], np.concatenate(lists))
                small, counts2 = pfind_batch(pats, pt, off=off, n=ln, cap=total - 1)
                assert small is None and np.array_equal(counts2, ref_counts)
    assert compared == 2 * 2 * 64


@pytest.mark.parametrize("sigma", [4, 2])
def test_against_the_byte_text_at_size(sigma):
    n = 1 << 30
    text = Text.generate(0x5EED0300 + sigma, sigma, n)
    compared = 0
    ms = (4, 8, 32, 256, 4096) if sigma == 4 else (8, 32, 256, 4096)  # rand2 m = 4: ~64 Mi positions
    try:
        with PackedText.pack(text) as pt:
            for m in ms:
                for k in (0, 123456789, n // 2 + 31, n - m):
                    P = text.read(k, m)
                    got, count = pfind(P, pt, cap=8 << 20)
                    want, wc = smart_amd.find(P, text, cap=8 << 20)
                    print("sigma=%d m=%d k=%d count=%d want=%d" % (sigma, m, k, count, wc))
                    assert got is not None and want is not None
                    assert got.dtype == np.uint64 and np.array_equal(got, want)
                    assert count == wc == len(got) == psearch(P, pt)[0] and count >= 1
                    assert k in got
                    compared += 1
    finally:
        text.free()
    assert compared == 4 * len(ms)


def test_beyond_2_to_the_32_positions():
    """The seed: the first of 0x5EED0308 + i for which smart_amd.find on the BYTE text lists the 16 symbols at 2^32 + 5 on
    both sides of 2^32 (0x5EED0308 itself holds them once; 0x5EED0309: at 2391732567, 4294967301, 5225560427, 6476517965)."""
    n = 8 << 30
    text = Text.generate(0x5EED0309, 4, n)
    compared = 0
    try:
        with PackedText.pack(text) as pt:
            assert len(pt) == n and pt.planes == 2
            k = (1 << 32) + 5
            P = text.read(k, 16)
            got, count = pfind(P, pt)
            want, wc = smart_amd.find(P, text)
            print("8 Gi m=16 count=%d positions=%s" % (count, got.tolist()))
            assert got.dtype == np.uint64 and np.array_equal(got, want)
            assert count == wc == len(got) == psearch(P, pt)[0] and count >= 1
            assert k in got.tolist()
            assert int(got[0]) < (1 << 32) and int(got[-1]) > (1 << 32), got.tolist()  # entries on both sides of 2^32
            compared += 1
            for off in ((1 << 32) - (1 << 19), n - (1 << 20)):
                S = text.read(off, 1 << 20)
                for m in (3, 9, 16, 40):
                    Q = S[(1 << 19) - 4:(1 << 19) - 4 + m]
                    want = positions_by_definition(Q, S) + np.uint64(off)
                    compared += check(Q, pt, want, off=off, ln=1 << 20)
                    if off < (1 << 32) and m == 3:
                        assert int(want[0]) < (1 << 32) < int(want[-1])
    finally:
        text.free()
    assert compared == 9


FUZZ_CASES = 5000


def test_differential_fuzz():
    """5,000 random (value set, n <= 65,536, kind, off, len, m) cases from one seed, the generator of the counting fuzz;
    cap drawn per case from {count, count + 7, max(count - 1, 0), 0}: return code, count, and the list when complete."""
    rng = np.random.default_rng(0x9A7E5)
    ran = complete = short = 0
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
        want = positions_by_definition(P, T, off, ln)
        count = len(want)
        cap = (count, count + 7, max(count - 1, 0), 0)[int(rng.integers(0, 4))]
        with PackedText.upload(T) as pt:
            rc, c, buf = pfind_c(P, pt, off, ln, cap, guard=2)
        info = dict(case=case, vals=vals.tolist(), n=n, kind=kind, off=off, len=ln, m=m, cap=cap, rc=rc, got=c, want=count)
        assert c == count, info
        assert rc == (OK if count <= cap else ERR_NOMEM), info
        assert np.all(buf[cap:] == np.uint64(0xDEADBEEFDEADBEEF)), info
        if count <= cap:
            assert np.array_equal(buf[:count], want), info
            complete += 1
        else:
            short += 1
        ran += 1
        if ran % 1000 == 0:
            print("fuzz: %d cases, %d complete lists" % (ran, complete), flush=True)
    assert ran == FUZZ_CASES == 5000
    assert complete > 0 and short > 0


def test_counting_is_untouched_by_finds():
    """psearch of the same patterns before and after finds on the same text: nothing is left behind in the cursor (the
    counting batch's first result slot) or the staging slots."""
    T = random_text((65, 67, 71, 84), 2**20 + 77, 9000)
    T[5000:9000] = 65
    pats = [T[k:k + m].copy() for m in (1, 3, 8, 33, 500) for k in (0, 5100, 700000)]
    with PackedText.upload(T) as pt:
        before = [psearch(P, pt)[0] for P in pats]
        batch_before = {m: psearch_batch([P for P in pats if len(P) == m], pt)[0].tolist() for m in (1, 3, 8, 33, 500)}
        for P, c in zip(pats, before):
            got, count = pfind(P, pt, cap=c + 1)
            assert count == c and np.array_equal(got, positions_by_definition(P, T))
            assert psearch(P, pt)[0] == c              # right after the find
            assert pfind(P, pt, cap=0)[1] == c         # a find that drops every entry
            assert psearch(P, pt, off=3, n=70000)[0] == len(positions_by_definition(P, T, 3, 70000))
        for m in (1, 3, 8, 33, 500):
            group = [P for P in pats if len(P) == m]
            lists, counts = pfind_batch(group, pt, cap=4 << 20)
            assert counts.tolist() == batch_before[m] == [len(x) for x in lists]
            assert psearch_batch(group, pt)[0].tolist() == batch_before[m]
        assert [psearch(P, pt)[0] for P in pats] == before
