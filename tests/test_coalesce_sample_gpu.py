"""hor_sample_scan on the GPU: shared passes of patterns of 31 bytes and more over the text's SAMPLE (the 4 bytes at every
28th position, smart_amd/csrc/sample.hpp, k_hors.hip), through the C ABI, against the oracle's brute force.  Bit-exact.

Texts of 3 MiB with smartgpu_text_sampling(0) and a sampled pass of TWO workgroups (smartgpu_coalesce_sample_grid): each
walks 14 rows of 4096 samples, four steps of its loop with a short last one.  Per length (31, 32, 33, 58, 59, 60, 64,
65, 66, 256): a copy of one pattern at every residue of s mod 28, at s = 0 and at s = n - m, the same pattern twice in
the pass, two patterns whose first 31 bytes agree, a pattern and its one-byte shift, a run of period 5 with a pattern
from it; bytes of 128 and more; m = 30 stays with hor_multi_scan; passes of 2, 84, 85 (the narrowest long pass) and 252
patterns; three shards that overlap by m - 1; a text created with sampling off; sampled passes switched off at m = 32,
64 and 256; m = 4096; and one text just above 2^32 bytes, where the sampled pass and hor_multi_scan must agree."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from smart_amd import Plan, Text, engine  # noqa: E402
from test_coalesce_gram_gpu import need_gpu, streaming  # noqa: E402,F401

SEED = 0x5EED5A3B
N = 3 << 20
MS = (31, 32, 33, 58, 59, 60, 64, 65, 66, 256)
STEP = 28 * 1500  # between planted copies: a multiple of 28, so copy r lies at residue (BASE + r) mod 28
BASE = 100_000


@pytest.fixture(autouse=True)
def every_text_sampled_two_workgroups():
    width = engine.coalesce_pass(engine.PASS_MAX)
    least = engine.coalesce_long(0)
    sampling = engine.text_sampling(0)
    grid = engine.coalesce_sample_grid(2)
    on = engine.coalesce_sample(True)
    try:
        yield
    finally:
        engine.device_sync(0)
        engine.coalesce_sample(on)
        engine.coalesce_sample_grid(grid)
        engine.text_sampling(sampling)
        engine.coalesce_long(least)
        engine.coalesce_pass(width)


def cut(T, at, m):
    """The first streaming pattern of m bytes at or after T[at] (below 32 bytes one window in ten is one)."""
    for d in range(4000):
        P = T[at + d:at + d + m].copy()
        if streaming(P):
            return P
    raise AssertionError("no streaming pattern near %d" % at)


def build(po, m, sigma=128, n=N, npats=24):
    """-> (T, pats): pats[0] planted at every residue, at 0 and at n - m; pats[1] == pats[2]; pats[3], pats[4] agree in
    their first m - 1 bytes; pats[6] is pats[5] shifted by one byte; pats[-1] comes from a run of period 5."""
    T = po.gen_text(SEED + m + sigma, sigma, 0, n).copy()
    fresh = po.gen_text(SEED + 31 * m + sigma, sigma, 0, n)
    pats = [cut(fresh, 1000 + 4001 * j, m) for j in range(npats - 1)]
    pats[2] = pats[1].copy()
    pats[4] = pats[3].copy()
    pats[4][m - 1] ^= 1
    at6 = BASE + 40 * STEP
    T[at6:at6 + m] = pats[5]
    pats[6] = T[at6 + 1:at6 + 1 + m].copy()
    assert streaming(pats[4]) and streaming(pats[6])
    for r in range(28):
        T[BASE + r * STEP + r:BASE + r * STEP + r + m] = pats[0]
    T[:m] = pats[0]
    T[n - m:] = pats[0]
    for j in range(1, npats - 1):
        if j != 6:
            at = BASE + (41 + j) * STEP + 3 * j
            T[at:at + m] = pats[j]
    run = np.frombuffer((b"abcab" * (m // 5 + 8)), dtype=np.uint8)
    T[2_000_000:2_000_000 + 6 * m] = np.resize(run[:5], 6 * m)
    pats.append(T[2_000_005:2_000_005 + m].copy())
    return T, pats


class Run:
    def __init__(self, po, T, pats, want=None):
        self.T, self.pats = T, pats
        self.want = [po.search("bf", P, T) for P in pats] if want is None else want
        self.text = Text.upload(T)
        self.plans = [Plan("hor", P) for P in pats]

    def launch(self, order, off=0, n=None):
        """-> (counts per plan, passes sent, sampled passes sent)"""
        for pl in self.plans:
            pl.reset()
        engine.device_sync(0)
        p0, s0 = engine.coalesce_stats(0)[1], engine.coalesce_sampled(0)
        for j in order:
            self.plans[j].launch(self.text, off=off, n=len(self.T) - off if n is None else n)
        engine.device_sync(0)
        return [pl.result(0)[0] for pl in self.plans], engine.coalesce_stats(0)[1] - p0, engine.coalesce_sampled(0) - s0

    def free(self):
        for pl in self.plans:
            pl.free()
        self.text.free()


_runs = {}


@pytest.fixture
def run(oracle):
    def get(m, sigma=128):
        if (m, sigma) not in _runs:
            T, pats = build(oracle, m, sigma)
            _runs[(m, sigma)] = Run(oracle, T, pats)
        return _runs[(m, sigma)]
    return get


@pytest.mark.parametrize("m", MS)
def test_counts_like_brute_force(run, m):
    r = run(m)
    assert engine.text_has_sample(r.text)
    assert r.want[0] >= 30 and r.want[1] == r.want[2] >= 1 and r.want[3] >= 1 and r.want[4] >= 1 and r.want[5] >= 1 and r.want[6] >= 1 and r.want[-1] >= 5
    order = list(range(len(r.pats)))
    got, passes, sampled = r.launch(order)
    assert got == r.want, (m, got, r.want)
    assert sampled == 1 and passes <= 2  # (the pattern of period 5 rides, or goes alone where it may not)
    got, _, sampled = r.launch(order[::-1][1:])  # other slots, other entries
    assert got == r.want[:-1] + [0] and sampled == 1
    engine.coalesce_sample_grid(0)  # one workgroup per compute unit
    got, _, sampled = r.launch(order)
    assert got == r.want and sampled == 1


@pytest.mark.parametrize("m", (32, 59, 256))
def test_byte_values_of_128_and_more(run, m):
    r = run(m, sigma=256)
    assert max(int(P.max()) for P in r.pats) >= 128
    got, _, sampled = r.launch(range(len(r.pats)))
    assert got == r.want and sampled == 1


def test_patterns_of_30_bytes_stay_with_hor_multi_scan(oracle):
    T = oracle.gen_text(SEED + 30, 128, 0, 1 << 20).copy()
    pats = [cut(T, 5000 + 9001 * j, 30) for j in range(8)]
    r = Run(oracle, T, pats)
    try:
        assert engine.text_has_sample(r.text)
        got, passes, sampled = r.launch(range(8))
        assert got == r.want and min(got) >= 1 and passes == 1 and sampled == 0
    finally:
        r.free()


@pytest.mark.parametrize("m", (32, 64))
def test_pass_widths(run, m):
    """2, 84 (a full by-value pass), 84 + 85 (the narrowest long pass behind it), 84 + 252 (a full long pass), and two more."""
    r = run(m)
    k = len(r.pats) - 1  # without the rider: every launch counts toward the width
    W, LW = engine.SAMPLE_WIDTH, engine.SAMPLE_LONG_WIDTH
    for launches, passes in ((2, 1), (W, 1), (W + W + 1, 2), (W + LW, 2), (W + LW + 2, 3)):
        order = [j % k for j in range(launches)]
        got, sent, sampled = r.launch(order)
        assert got[:k] == [w * order.count(j) for j, w in enumerate(r.want[:k])], (m, launches)
        assert sent == sampled == passes, (m, launches, sent, sampled)


@pytest.mark.parametrize("m", (31, 64))
def test_three_shards_sum_to_the_whole(run, m):
    r = run(m)
    n = len(r.T)
    cuts = [0, n // 3 + 5, 2 * n // 3 + 17, n]
    total = [0] * len(r.pats)
    for lo, hi in zip(cuts, cuts[1:]):
        hi = min(n, hi + m - 1)
        got, _, sampled = r.launch(range(len(r.pats)), off=lo, n=hi - lo)
        assert sampled == 1
        total = [a + b for a, b in zip(total, got)]
    assert total == r.want


@pytest.mark.parametrize("m", (32, 60))
def test_sub_ranges_that_begin_inside_a_gram(run, oracle, m):
    """Ranges whose ends are no multiples of 28: one start position exactly on a planted copy, the one behind it, and wider ones."""
    r = run(m)
    at = BASE + 5 * STEP + 5  # the copy at residue (BASE + 5) mod 28
    for off, n in ((at, m), (at + 1, m), (at - 1, m + 2), (29, m), (27, len(r.T) - 27), (BASE + 1, 3 * STEP + 1), (len(r.T) - m - 3, m + 3)):
        want = [oracle.search("bf", P, r.T[off:off + n]) for P in r.pats]
        got, _, sampled = r.launch(range(len(r.pats)), off=off, n=n)
        assert got == want and sampled == 1, (m, off, n, got, want)
    assert oracle.search("bf", r.pats[0], r.T[at:at + m]) == 1


@pytest.mark.parametrize("m", (32, 33, 59, 64))
def test_the_shortest_texts(oracle, m):
    """n = m, m + 1, 55, 56, 57 and 28 k +- 1: a pattern from the front and one from the back of each text."""
    ns = sorted({m, m + 1, 55, 56, 57} | {28 * k + d for k in range(2, 6) for d in (-1, 1)})
    for n in [n for n in ns if n >= m]:
        seed = SEED + 977 * n
        while True:
            T = oracle.gen_text(seed, 128, 0, n).copy()
            if streaming(T[:m]) and streaming(T[n - m:]):
                break
            seed += 8 * n
        r = Run(oracle, T, [T[:m].copy(), T[n - m:].copy()])
        try:
            assert engine.text_has_sample(r.text)
            got, passes, sampled = r.launch([0, 1])
            assert got == r.want and min(got) >= 1 and passes == sampled == 1, (m, n, got, r.want)
        finally:
            r.free()


def test_a_text_created_with_sampling_off_has_no_sample(run, oracle):
    r = run(32)
    engine.text_sampling(-1)
    text = Text.upload(r.T)
    engine.text_sampling(0)
    try:
        assert not engine.text_has_sample(text)
        sampled, text_with = r, r.text
        r.text = text
        try:
            got, passes, n_sampled = r.launch(range(len(r.pats)))
        finally:
            r.text = text_with
        assert got == sampled.want and n_sampled == 0 and passes >= 1
    finally:
        text.free()


@pytest.mark.parametrize("m", (32, 64, 256))
def test_sampled_passes_switched_off(run, m):
    r = run(m)
    assert engine.coalesce_sample(False) is True
    got, passes, sampled = r.launch(range(len(r.pats)))
    assert got == r.want and sampled == 0 and passes >= 1
    assert engine.coalesce_sample(True) is False
    got, _, sampled = r.launch(range(len(r.pats)))
    assert got == r.want and sampled == 1


def test_windows_of_4096_bytes(oracle):
    m, n = 4096, 1 << 20
    T = oracle.gen_text(SEED + m, 128, 0, n).copy()
    pats = [T[50_000 * j + 7 * j:50_000 * j + 7 * j + m].copy() for j in range(1, 9)]
    pats.append(pats[0].copy())
    pats[-1][m - 1] ^= 1  # agrees with pats[0] up to its last byte
    T[900_000:900_000 + m] = pats[-1]
    T[n - m:] = pats[1]
    r = Run(oracle, T, pats)
    try:
        got, _, sampled = r.launch(range(len(pats)))
        assert got == r.want and r.want[1] == 2 and r.want[-1] == 1 and sampled == 1
    finally:
        r.free()


def test_beyond_two_to_the_32(oracle):
    """4 GiB + 3 MiB of rand128: eight patterns of 32 bytes read from the text, two of them from beyond 2^32 and one at
    n - m; the sampled pass and hor_multi_scan must agree, and every count is at least 1."""
    engine.coalesce_sample_grid(0)
    n, m = (1 << 32) + (3 << 20), 32
    text = Text.generate(SEED, 128, n)
    plans = []
    try:
        assert engine.text_has_sample(text)
        places = [0, 123_457, (1 << 31) - 16, (1 << 31) + 5, (1 << 32) - 20, (1 << 32) + 1, (1 << 32) + (2 << 20) + 13, n - m]
        pats = [text.read(at, m) for at in places]
        assert all(streaming(P) for P in pats)
        plans = [Plan("hor", P) for P in pats]
        counts = {}
        for on in (True, False):
            engine.coalesce_sample(on)
            for pl in plans:
                pl.reset()
            engine.device_sync(0)
            s0 = engine.coalesce_sampled(0)
            for pl in plans:
                pl.launch(text)
            engine.device_sync(0)
            counts[on] = [pl.result(0)[0] for pl in plans]
            assert engine.coalesce_sampled(0) - s0 == (1 if on else 0)
        assert counts[True] == counts[False] and min(counts[True]) >= 1, counts
    finally:
        for pl in plans:
            pl.free()
        text.free()


def test_free_the_shared_texts():
    for r in _runs.values():
        r.free()
    _runs.clear()
