"""The walk of hor_multi_scan (k_horm.hip): a lane goes through ALL patterns of a pass in one loop over (pattern,
window end), in one, two or four chains that each take a contiguous share of the patterns.  What that form can get
wrong and tests/test_coalesce_gpu.py (copies of ONE pattern) does not exercise:

* copies of TWO patterns of a group ending in one 64-byte lane segment of one tile, the two taken at group positions
  (0, 1), (0, 7) and (3, 4): the same chain and different chains at two and at four chains;
* completion in memory (m = 300) of two different patterns parked in neighbouring lanes of one wave — one wave-wide
  compare, two pattern pointers — and a lane that parks one candidate and completes another on the spot;
* groups of 2, 3, 5, 7 and 8 (sizes the number of chains does not divide) on a text shorter than a tile and on patterns
  that live in the last, partial tile of a four-tile text, where most lanes have no window end at all;
* one occurrence of the LAST pattern of a group of eight at position 0 and one at n - m.

Every count against the oracle's brute force and against the same launches under smartgpu_coalesce(0).  Bit-exact.
Texts: rand128 of 3 * 16384 + 777 bytes and of 5000 bytes.  The helpers are those of tests/test_coalesce_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Plan, Text, engine  # noqa: E402

TILE = 16384
N_BIG, N_SMALL = 3 * TILE + 777, 5000
SEED = 0x5EEDC0A2
PAIRS = ((0, 1), (0, 7), (3, 4))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


@pytest.fixture(autouse=True)
def groups_of_eight():
    """Every test starts with passes of up to eight launches, whatever the library's default is, and leaves that default behind."""
    default = engine.coalesce(8)
    yield
    engine.device_sync(0)
    engine.coalesce(default)


def streaming(P):
    """True for a pattern whose Horspool plan takes hor_scan's streaming form: its symbols do not repeat, by the rule of
    plan.cpp build_blob (ordered pairs of equal symbols against 1/48 of all pairs; below 32 bytes, four such pairs)."""
    m = len(P)
    c = np.bincount(P, minlength=256).astype(np.int64)
    pairs = int((c * (c - 1)).sum())
    repeats = m > 7 and (pairs * 48 > m * (m - 1) or (m < 32 and pairs >= 4))
    return not repeats and engine.kernel_for("hor", P) == "hor_scan"


def cut(T, k, m, reach=64):
    """The first streaming pattern of m bytes at or after T[k]."""
    for d in range(reach):
        P = T[k + d:k + d + m].copy()
        if len(P) == m and streaming(P):
            return P
    raise AssertionError("no streaming pattern near %d" % k)


def plant(T, taken, end, P):
    """Copy P into T with its last byte at T[end]; the copies of a text do not overlap."""
    lo = end - len(P) + 1
    assert lo >= 0 and end < len(T) and all(hi < lo or end < a for a, hi in taken), (lo, end, taken)
    taken.append((lo, end))
    T[lo:end + 1] = P


class Case:
    """One edited text with the patterns of its group, their plans and their brute-force counts (computed once)."""

    def __init__(self, po, T, pats):
        self.T, self.n, self.pats = T, len(T), pats
        self.want = [po.search("bf", P, T) for P in pats]
        self.text = Text.upload(T)
        self.plans = [Plan("hor", P) for P in pats]
        for pl in self.plans:
            assert pl.kernel_name == "hor_scan"

    def run(self, order):
        """Launch the plans `order` (indices), one sync; -> (counts in that order, kernels sent)."""
        for pl in self.plans:
            pl.reset()
        engine.device_sync(0)
        _, p0 = engine.coalesce_stats(0)
        for j in order:
            self.plans[j].launch(self.text)
        engine.device_sync(0)
        _, p1 = engine.coalesce_stats(0)
        return [self.plans[j].result(0)[0] for j in order], p1 - p0

    def check(self, order):
        """One shared pass and one launch per plan give the brute-force counts."""
        want = [self.want[j] for j in order]
        engine.coalesce(8)
        got, passes = self.run(order)
        assert got == want, (self.n, len(self.pats[0]), list(order), got, want)
        assert passes == 1 if len(order) <= 8 else passes < len(order)
        engine.coalesce(0)
        got, passes = self.run(order)
        assert got == want and passes == len(order), (self.n, len(self.pats[0]), list(order), got, want)
        engine.coalesce(8)


_cases = {}


def cached(key, make):
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def spread(T, m, count, lo, hi):
    """`count` streaming patterns cut from T[lo:hi) at even distances."""
    step = max(1, (hi - lo - m - 64) // count)
    return [cut(T, lo + j * step, m) for j in range(count)]


# --- several patterns in one lane segment ----------------------------------------------------------------------------
TWO_ENDS = {16: (20, 40), 17: (20, 40), 18: (20, 38), 32: (31, 63)}  # offsets of the two window ends in the segment


def make_segment_case(po, n, m):
    T = po.gen_text(SEED + m, 128, 0, n).copy()
    pats = spread(T, m, 8, 100, n - 100)
    taken = []
    qs = (150, 300, 600) if n == N_BIG else (20, 40, 60)  # big text: one segment in each of the first three tiles
    a, b = TWO_ENDS[m]
    for q, (i, j) in zip(qs, PAIRS):
        plant(T, taken, 64 * q + a, pats[i])
        plant(T, taken, 64 * q + b, pats[j])
    for P in pats:  # the edits left every pattern what it was cut as: at least its planted copies are there
        assert streaming(P)
    c = Case(po, T, pats)
    assert c.want[0] >= 2 and c.want[3] >= 1 and c.want[4] >= 1 and c.want[7] >= 1 and c.want[1] >= 1
    return c


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
@pytest.mark.parametrize("m", sorted(TWO_ENDS))
def test_two_patterns_end_in_one_lane_segment(oracle, n, m):
    c = cached(("seg", n, m), lambda: make_segment_case(oracle, n, m))
    c.check(range(8))


# --- completion in memory: two patterns parked in one wave, and a lane with two candidates -------------------------
def make_wave_case(po, n):
    m = 300
    T = po.gen_text(SEED + m, 128, 0, n).copy()
    # R: 364 bytes whose first and last 300 are both streaming patterns
    for k in range(700, 1200):
        R = T[k:k + 364].copy()
        if streaming(R[:300]) and streaming(R[64:]):
            break
    else:
        raise AssertionError("no region R")
    A, B = R[:300].copy(), R[64:].copy()
    taken = [(k, k + 363)]
    # R once more: A ends in lane 100 and B in lane 101 of one tile — neighbours in the second wave of the workgroup
    base = TILE if n == N_BIG else 0
    r_end = base + 64 * 101 + 5 if n == N_BIG else 64 * 37 + 5  # small text: lanes 36 and 37 of the first wave
    plant(T, taken, r_end, R)
    # A a second time, and D cut from the text 20 bytes further on: D's copy ends 20 bytes behind A's in the same lane
    # segment, so that lane has two candidates in one tile — it parks the one it meets first and completes the other
    a2_end = base + 64 * 180 + 10 if n == N_BIG else 64 * 60 + 10
    plant(T, taken, a2_end, A)
    D = T[a2_end + 20 - m + 1:a2_end + 20 + 1].copy()
    assert (a2_end + 20) // 64 == a2_end // 64 and streaming(D)
    taken[-1] = (taken[-1][0], a2_end + 20)
    others = spread(T, m, 5, 100, n - 10)
    pats = [A, B, D] + others
    assert len(pats) == 8
    c = Case(po, T, pats)
    assert c.want[0] >= 3 and c.want[1] >= 2 and c.want[2] >= 1, c.want[:3]
    return c


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
def test_completion_in_memory_of_two_patterns_in_one_wave(oracle, n):
    c = cached(("wave", n), lambda: make_wave_case(oracle, n))
    c.check(range(8))
    c.check((2, 1, 0, 3, 4, 5, 6, 7))  # D before A: the lane parks the other candidate
    c.check((3, 4, 5, 0, 6, 7, 1, 2))  # A, B and D in different chains
    c.check((0, 1))
    c.check((2, 0, 1))


# --- group sizes ---------------------------------------------------------------------------------------------------
def make_sizes_case(po, n, m):
    T = po.gen_text(SEED + 1000 + m, 128, 0, n).copy()
    if n == N_BIG:  # patterns of the last, partial tile: 777 bytes, lanes 13.. of its first wave have no window end
        lo, hi = 3 * TILE + 8, n
        step = (hi - lo - m - 16) // 8
        assert step >= 1
        pats = [cut(T, lo + j * step, m, reach=min(step, 16)) for j in range(8)]
    else:
        pats = spread(T, m, 8, 50, n - 50)
    return Case(po, T, pats)


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
@pytest.mark.parametrize("m", (16, 32, 300))
def test_group_sizes(oracle, n, m):
    c = cached(("sizes", n, m), lambda: make_sizes_case(oracle, n, m))
    assert min(c.want) >= 1
    for k in (2, 3, 5, 7, 8):
        c.check(range(k))
        c.check(range(8 - k, 8))


# --- first and last position ---------------------------------------------------------------------------------------
def make_ends_case(po, n, m):
    T = po.gen_text(SEED + 2000 + m, 128, 0, n).copy()
    pats = spread(T, m, 8, 400, n - 400)
    taken = []
    plant(T, taken, m - 1, pats[7])
    plant(T, taken, n - 1, pats[7])
    c = Case(po, T, pats)
    assert c.want[7] >= 3 and np.array_equal(T[:m], pats[7]) and np.array_equal(T[n - m:], pats[7])
    return c


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
@pytest.mark.parametrize("m", (16, 18, 32, 300))
def test_last_pattern_at_the_first_and_the_last_position(oracle, n, m):
    c = cached(("ends", n, m), lambda: make_ends_case(oracle, n, m))
    c.check(range(8))
    # the occurrences at 0 and at n - m alone: a range without them counts two fewer
    for pl in c.plans:
        pl.reset()
    for pl in c.plans:
        pl.launch(c.text, off=1, n=c.n - 2)
    engine.device_sync(0)
    inner = [oracle.search("bf", P, c.T[1:c.n - 1]) for P in c.pats]
    assert [pl.result(0)[0] for pl in c.plans] == inner and inner[7] == c.want[7] - 2
