"""Positions of a pattern set on a byte text (smartgpu_find_batch64, k_hormf.hip's hor_multi_find) on the GPU, against a
bytes.find loop per pattern over the range; bit-exact.

The base text is 3 * 16384 + 300 bytes with the range starting at off = 129: three tiles and a ragged last one, and a range
that begins in the middle of a lane's segment — the smallest shape that crosses every border of the kernel."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Plan, Text, engine  # noqa: E402

TILE = 16384
N_TEXT = 3 * TILE + 300
OFF = 129
N_RANGE = N_TEXT - OFF - 40  # the range ends 40 bytes before the text does
MS = (3, 4, 8, 16, 17, 18, 32, 48, 49, 64, 65, 100, 300)
OK, ERR_ARG, ERR_NOMEM = 0, -3, -5
SENTINEL = 0xDEADBEEFCAFEF00D


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def reference(T, pats, off, n):
    """The definition: for every pattern the ascending starts s in [off, off + n - m] with T[s : s + m] == P, by bytes.find."""
    hay = T.tobytes()
    out = []
    for P in pats:
        needle, m = P.tobytes(), len(P)
        found, s = [], hay.find(needle, off)
        while s != -1 and s + m <= off + n:
            found.append(s)
            s = hay.find(needle, s + 1)
        out.append(np.array(found, dtype=np.uint64))
    return out


def raw(pats, text, off, n, cap, positions=True, tail=4):
    """smartgpu_find_batch64 itself: (rc, the `cap` + `tail` entries of the positions buffer, starts).  The buffer is filled
    with SENTINEL before the call."""
    pats = [np.ascontiguousarray(p, dtype=np.uint8) for p in pats]
    K = len(pats)
    ptrs = (ctypes.c_void_p * K)(*[p.ctypes.data for p in pats])
    out = np.full(cap + tail, SENTINEL, dtype=np.uint64)
    starts = np.full(K + 1, SENTINEL, dtype=np.uint64)
    rc = engine.lib().smartgpu_find_batch64(ctypes.cast(ptrs, ctypes.c_void_p), len(pats[0]), K, text._h, off, n,
                                            out.ctypes.data if positions else None, cap, starts.ctypes.data)
    return rc, out, starts


def check_against(want, rc, out, starts, cap, what):
    counts = [len(w) for w in want]
    assert rc == OK, (what, rc, engine.lib().smartgpu_last_error().decode())
    assert starts.tolist() == np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64).tolist(), what
    for k, w in enumerate(want):
        got = out[int(starts[k]):int(starts[k + 1])]
        assert np.array_equal(got, w), (what, k, got[:8], w[:8])
    assert (out[int(starts[-1]):] == SENTINEL).all(), what


# ---- lengths and widths --------------------------------------------------------------------------------------------------

def planted_ends(m):
    """Window ends of the planted copies: the last byte of a tile, the first of the next, the second of the one after, and
    either side of a 64-byte lane border.  They lie in distinct regions for every m of MS."""
    ends = [TILE - 1, 2 * TILE, 3 * TILE + 1, 64 * 100 - 1, 64 * 110, 64 * 120 + 1]
    spans = sorted((e - m + 1, e) for e in ends)
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])) and spans[0][0] > OFF + m and spans[-1][1] < OFF + N_RANGE
    return ends


class LengthCase:
    """The edited base text of one length with 2 W(m) + 3 patterns that all occur, their reference and their find()."""

    def __init__(self, m):
        self.m, self.W = m, engine.find_width(m)
        rng = np.random.default_rng(0xF1BA7C00 + m)
        T = rng.integers(0, 128, N_TEXT, dtype=np.uint8)
        ends = planted_ends(m)
        # the planted patterns are cut from a region that no copy touches
        planted = [T[20000 + 400 * j:20000 + 400 * j + m].copy() for j in range(len(ends))]
        for e, P in zip(ends, planted):
            T[e - m + 1:e + 1] = P
        last = OFF + N_RANGE - m
        special = [T[OFF:OFF + m].copy(),            # the first window of the range
                   T[last:last + m].copy(),          # the last
                   T[OFF - 1:OFF - 1 + m].copy(),    # a copy that begins one byte before the range: not listed there
                   T[last + 1:last + 1 + m].copy()]  # a copy that ends one byte behind it: not listed there
        K = 2 * self.W + 3
        cuts = rng.integers(OFF, last + 1, K - len(special) - len(planted))
        self.pats = special + planted + [T[c:c + m].copy() for c in cuts]
        self.T, self.text = T, Text.upload(T)
        self.want = reference(T, self.pats, OFF, N_RANGE)
        assert all(len(w) >= 1 for w in self.want[:2] + self.want[4:])  # every pattern occurs (two only outside the range, unless by chance)
        if m >= 8:
            assert len(self.want[2]) == 0 and len(self.want[3]) == 0
        for e, w in zip(ends, self.want[4:]):
            assert e - m + 1 in w.tolist()


_length_cases = {}


def length_case(m):
    if m not in _length_cases:
        _length_cases[m] = LengthCase(m)
    return _length_cases[m]


@pytest.mark.parametrize("m", MS)
def test_lengths_and_widths(m):
    c = length_case(m)
    for K in (1, 2, c.W, c.W + 1, 2 * c.W + 3):  # a pass of one, a full pass, a full pass and one, three passes on one cursor
        pats, want = c.pats[:K], c.want[:K]
        total = sum(len(w) for w in want)
        rc, out, starts = raw(pats, c.text, OFF, N_RANGE, total)
        check_against(want, rc, out, starts, total, (m, K))
        counts = engine.search_batch("hor", pats, c.text, OFF, N_RANGE, per_pattern_times=False)[0]
        assert counts.tolist() == np.diff(starts).tolist(), (m, K)
    # each slice is find() of its pattern (the largest set holds the others)
    for k, P in enumerate(c.pats):
        pos, cnt = engine.find(P, c.text, OFF, N_RANGE)
        assert cnt == len(c.want[k]) and np.array_equal(pos, c.want[k]), (m, k)


# ---- bytes >= 128, dense chains, the same pattern several times ------------------------------------------------------------

def test_bytes_above_127_and_a_chain_of_fifty():
    rng = np.random.default_rng(0xF1BA7C50)
    T = rng.integers(0, 256, N_TEXT, dtype=np.uint8)
    m = 24
    pats = []
    for j in range(50):  # fifty patterns whose last two bytes are the same: one bucket chain of fifty links
        P = T[1000 + 300 * j:1000 + 300 * j + m].copy()
        P[-2:] = (0xC3, 0x91)
        T[25000 + 100 * j:25000 + 100 * j + m] = P
        T[45000 + 64 * j:45000 + 64 * j + 2] = (0xC3, 0x91)  # and the gram alone, for every pattern of the chain to die on
        pats.append(P)
    pats += [pats[7]] * 8  # eight identical patterns
    pats += [T[c:c + m].copy() for c in rng.integers(OFF, N_TEXT - m - 40, 30)]
    want = reference(T, pats, OFF, N_RANGE)
    assert all(len(w) >= 1 for w in want) and (T >= 128).sum() > N_TEXT // 3
    text = Text.upload(T)
    total = sum(len(w) for w in want)
    rc, out, starts = raw(pats, text, OFF, N_RANGE, total)
    check_against(want, rc, out, starts, total, "rand256")
    for k in range(50, 58):
        assert np.array_equal(out[int(starts[k]):int(starts[k + 1])], want[7]) and len(want[7]) >= 1


# ---- frequent occurrences: the stage fills in every tile and lanes take the overflow path ---------------------------------

@pytest.mark.parametrize("period", [1, 2])
@pytest.mark.parametrize("m", [4, 40])
def test_frequent_occurrences(period, m):
    n = 20000
    T = np.resize(np.array([0x61, 0x62][:period], dtype=np.uint8), n)
    pats = [T[:m].copy()] * 4
    want = reference(T, pats, 0, n)
    assert len(want[0]) == (n - m + 1 + period - 1) // period
    text = Text.upload(T)
    lists, counts = engine.find_batch(pats, text, cap=4 * len(want[0]))
    assert counts.tolist() == [len(want[0])] * 4
    for got in lists:
        assert np.array_equal(got, want[0])


# ---- cap -----------------------------------------------------------------------------------------------------------------

def test_cap():
    c = length_case(32)
    K = c.W + 1
    pats, want = c.pats[:K], c.want[:K]
    total = sum(len(w) for w in want)
    rc, out, starts = raw(pats, c.text, OFF, N_RANGE, total)
    check_against(want, rc, out, starts, total, "cap = total")
    rc, out1, starts1 = raw(pats, c.text, OFF, N_RANGE, total - 1)
    assert rc == ERR_NOMEM and "occurrences, room for" in engine.lib().smartgpu_last_error().decode()
    assert starts1.tolist() == starts.tolist()
    assert (out1[total - 1:] == SENTINEL).all()  # nothing behind positions[cap - 1]
    rc, out0, starts0 = raw(pats, c.text, OFF, N_RANGE, 0, positions=False)
    assert rc == ERR_NOMEM and starts0.tolist() == starts.tolist() and (out0 == SENTINEL).all()
    # a set that does not occur: cap = 0 with positions = NULL is a complete answer
    absent = [np.full(32, 200, dtype=np.uint8), np.full(32, 201, dtype=np.uint8)]
    rc, _, s = raw(absent, c.text, OFF, N_RANGE, 0, positions=False)
    assert rc == OK and s.tolist() == [0, 0, 0]
    # the Python wrapper: None and the counts
    lists, counts = engine.find_batch(pats, c.text, OFF, N_RANGE, cap=total - 1)
    assert lists is None and counts.tolist() == [len(w) for w in want]
    lists, counts = engine.find_batch(pats, c.text, OFF, N_RANGE, cap=total)
    assert counts.tolist() == [len(w) for w in want] and all(np.array_equal(g, w) for g, w in zip(lists, want))


# ---- m = 1, 2 and m > n --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2])
def test_short_patterns(m):
    c = length_case(32)
    pats = [c.T[k:k + m].copy() for k in (OFF, 5000, 5000, OFF + N_RANGE - m, OFF - 1)] + [np.full(m, 250, dtype=np.uint8)]
    want = reference(c.T, pats, OFF, N_RANGE)
    total = sum(len(w) for w in want)
    assert total >= 10 and all(len(w) >= 1 for w in want[:4]) and len(want[-1]) == 0
    rc, out, starts = raw(pats, c.text, OFF, N_RANGE, total)
    check_against(want, rc, out, starts, total, m)
    rc, out1, starts1 = raw(pats, c.text, OFF, N_RANGE, total - 1)
    assert rc == ERR_NOMEM and starts1.tolist() == starts.tolist() and (out1[total - 1:] == SENTINEL).all()
    rc, _, starts0 = raw(pats, c.text, OFF, N_RANGE, 0, positions=False)
    assert rc == ERR_NOMEM and starts0.tolist() == starts.tolist()


def test_pattern_longer_than_the_range():
    c = length_case(32)
    L = engine.lib()
    assert raw(c.pats[:3], c.text, N_TEXT, 1, 4)[0] == ERR_ARG  # leaves a message behind
    before = L.smartgpu_last_error()
    assert before
    for n in (0, 1, 31):
        rc, out, starts = raw(c.pats[:3], c.text, OFF, n, 4)
        assert rc == OK and starts.tolist() == [0, 0, 0, 0] and (out == SENTINEL).all()
        assert L.smartgpu_last_error() == before


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_argument_refusals():
    c = length_case(32)
    L = engine.lib()
    f = L.smartgpu_find_batch64
    pats = c.pats[:3]
    ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in pats])
    P = ctypes.cast(ptrs, ctypes.c_void_p)
    out = np.full(8, SENTINEL, dtype=np.uint64)
    starts = np.full(4, SENTINEL, dtype=np.uint64)

    def refused(rc, says):
        assert rc == ERR_ARG, rc
        assert says in L.smartgpu_last_error().decode(), (says, L.smartgpu_last_error().decode())

    h = c.text._h
    refused(f(None, 32, 3, h, OFF, N_RANGE, out.ctypes.data, 8, starts.ctypes.data), "P/starts NULL or K = 0")
    refused(f(P, 32, 3, h, OFF, N_RANGE, out.ctypes.data, 8, None), "P/starts NULL or K = 0")
    refused(f(P, 32, 0, h, OFF, N_RANGE, out.ctypes.data, 8, starts.ctypes.data), "P/starts NULL or K = 0")
    refused(f(P, 32, 3, None, OFF, N_RANGE, out.ctypes.data, 8, starts.ctypes.data), "text handle is NULL")
    refused(f(P, 32, 3, h, OFF, N_RANGE, None, 8, starts.ctypes.data), "positions NULL with cap > 0")
    refused(f(P, 32, 3, h, OFF, N_TEXT - OFF + 1, out.ctypes.data, 8, starts.ctypes.data), "outside the text")
    refused(f(P, 32, 3, h, N_TEXT + 1, 0, out.ctypes.data, 8, starts.ctypes.data), "outside the text")
    holed = (ctypes.c_void_p * 3)(pats[0].ctypes.data, None, pats[2].ctypes.data)
    refused(f(ctypes.cast(holed, ctypes.c_void_p), 32, 3, h, OFF, N_RANGE, out.ctypes.data, 8, starts.ctypes.data), "pattern 1 is NULL")
    # K beyond what the staging buffer holds at this length, and beyond 2^18
    long_pat = np.zeros(300, dtype=np.uint8)
    bound = engine.find_batch_max(300)
    many = (ctypes.c_void_p * (bound + 1))(*([long_pat.ctypes.data] * (bound + 1)))
    big_starts = np.full(bound + 2, SENTINEL, dtype=np.uint64)
    refused(f(ctypes.cast(many, ctypes.c_void_p), 300, bound + 1, h, OFF, N_RANGE, out.ctypes.data, 8, big_starts.ctypes.data),
            "%d patterns of length 300, at most %d per call" % (bound + 1, bound))
    refused(f(P, 32, (1 << 18) + 1, h, OFF, N_RANGE, out.ctypes.data, 8, starts.ctypes.data), "patterns in one set (at most 262144")
    assert (out == SENTINEL).all() and (starts == SENTINEL).all() and (big_starts == SENTINEL).all()  # a refused call writes nothing


# ---- after queued launches -----------------------------------------------------------------------------------------------

def test_after_queued_launches():
    """Coalesced Plan.launch calls that are still queued when find_batch is called: the call sends them first, and both the
    plans' counts and the lists are right."""
    c = length_case(32)
    whole = reference(c.T, c.pats, 0, N_TEXT)
    streaming = [k for k, P in enumerate(c.pats) if len(set(P.tolist())) >= 28 and engine.kernel_for("hor", P) == "hor_scan"][:5]
    assert len(streaming) == 5
    default = engine.coalesce(8)
    plans = [Plan("hor", c.pats[k]) for k in streaming]
    try:
        engine.device_sync(0)
        l0, p0 = engine.coalesce_stats(0)
        for pl in plans:
            pl.launch(c.text)
        K = c.W + 1
        lists, counts = engine.find_batch(c.pats[:K], c.text, OFF, N_RANGE)  # no synchronisation in between
        l1, p1 = engine.coalesce_stats(0)
        assert l1 - l0 == 5 and p1 - p0 < 5  # they were queued, and left as a shared pass
        assert [pl.result(0)[0] for pl in plans] == [len(whole[k]) for k in streaming]
        assert all(np.array_equal(g, w) for g, w in zip(lists, c.want[:K])) and counts.tolist() == [len(w) for w in c.want[:K]]
    finally:
        for pl in plans:
            pl.free()
        engine.device_sync(0)
        engine.coalesce(default)


# ---- mixed lengths ---------------------------------------------------------------------------------------------------------

def test_mixed_lengths():
    a = length_case(32)
    T = a.T
    rng = np.random.default_rng(0xF1BA7C33)
    pats = []
    for m in (300, 2, 32, 17, 32, 1, 65, 300, 17):
        k = int(rng.integers(OFF, OFF + N_RANGE - m))
        pats.append(T[k:k + m].copy())
    want = reference(T, pats, OFF, N_RANGE)
    lists, counts = engine.find_batch(pats, a.text, OFF, N_RANGE)
    assert counts.tolist() == [len(w) for w in want] and all(len(w) >= 1 for w in want)
    assert all(np.array_equal(g, w) for g, w in zip(lists, want))
    total = sum(len(w) for w in want)
    lists, counts = engine.find_batch(pats, a.text, OFF, N_RANGE, cap=total - 1)
    assert lists is None and counts.tolist() == [len(w) for w in want]
    lists, counts = engine.find_batch(pats, a.text, OFF, N_RANGE, cap=total)
    assert all(np.array_equal(g, w) for g, w in zip(lists, want))


# ---- a seeded differential loop --------------------------------------------------------------------------------------------

FUZZ_SEED = 0xF1BA7CF2


def test_differential_loop():
    """40 cases: m, K, the alphabet, the range and the plants drawn at random, against the same reference."""
    for case in range(40):
        rng = np.random.default_rng([FUZZ_SEED, case])
        sigma = int(rng.choice([2, 4, 20, 128, 256]))
        n_text = int(rng.integers(200, 3 * TILE if sigma >= 20 else 6000))  # (few values: short patterns occur everywhere)
        m = int(rng.choice([1, 2, 3, 4, 5, 9, 16, 17, 18, 19, 31, 32, 33, 47, 64, 65, 66, 129, 257]))
        m = min(m, n_text // 2)
        K = int(rng.choice([1, 2, 3, 7, 60, 130, 260]))
        T = rng.integers(0, sigma, n_text, dtype=np.uint8)
        off = int(rng.integers(0, n_text - m))
        n = int(rng.integers(0, n_text - off + 1))
        pats = []
        for _ in range(K):
            kind = int(rng.integers(0, 4))
            if kind == 0:  # absent, most likely
                pats.append(rng.integers(0, 256, m, dtype=np.uint8))
            else:          # cut from the text, and planted once more
                k = int(rng.integers(0, n_text - m + 1))
                P = T[k:k + m].copy()
                if kind == 2:
                    at = int(rng.integers(0, n_text - m + 1))
                    T[at:at + m] = P
                pats.append(P)
        want = reference(T, pats, off, n)
        total = sum(len(w) for w in want)
        what = "seed %#x case %d: sigma %d, text %d, m %d, K %d, range [%d, +%d), %d occurrences" % (FUZZ_SEED, case, sigma, n_text, m, K, off, n, total)
        text = Text.upload(T)
        rc, out, starts = raw(pats, text, off, n, total)
        check_against(want, rc, out, starts, total, what)
        text.free()
