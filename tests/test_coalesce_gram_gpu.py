"""The shared walk of hor_multi_scan (k_horm.hip): ONE walk per lane over a skip table that all patterns of a pass share,
indexed by a window's last two bytes (multi.hpp).  What that form can get wrong:

* a gram whose two bytes lie in different dwords, swizzle blocks, lane segments or tiles, and the byte in front of a
  lane's first window end (the halo): one pattern of a group of eight ends at each of the 64 offsets around every tile
  boundary, TILE * b - 32 + r;
* grams of different patterns in one table slot: two last grams and two inner grams edited into the same slot;
* three patterns with the same last two bytes that differ at byte m - 3: one slot, three candidates per window;
* m = 8 (the shortest that queues), 17 (H = m - 1), 18 (first completion in memory), 300, and 70, whose shifts are capped
  at 64: copies whose ends lie 65 (the pattern overlaps itself there) and 128 bytes apart;
* a range that starts and ends inside a lane segment, with a copy at its first and at its last start position;
* a Tuned BM plan and Horspool plans in one group.

Every count against the oracle's brute force and against the same launches under smartgpu_coalesce(0), one pass per
group.  Bit-exact.  Texts of 3 * 16384 + 777 and of 5000 bytes.  The helpers are those of tests/test_coalesce_walk_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Plan, Text, engine  # noqa: E402

TILE = 16384
N_BIG, N_SMALL = 3 * TILE + 777, 5000
SEED = 0x5EEDC0A3
CAP = 64  # multi.hpp kGramCap: no entry shifts a window end further


def slot(prev, last):
    """The table slot of the gram (prev, last), by the rule of multi.hpp gram_slot: 2048 slots, (37 * prev + last) mod 2048."""
    return (37 * int(prev) + int(last)) % 2048


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


def streaming(P, algo="hor"):
    """True for a pattern whose Horspool plan takes hor_scan's streaming form: its symbols do not repeat, by the rule of
    plan.cpp build_blob (ordered pairs of equal symbols against 1/48 of all pairs; below 32 bytes, four such pairs)."""
    m = len(P)
    c = np.bincount(P, minlength=256).astype(np.int64)
    pairs = int((c * (c - 1)).sum())
    repeats = m > 7 and (pairs * 48 > m * (m - 1) or (m < 32 and pairs >= 4))
    return not repeats and engine.kernel_for(algo, P) == "hor_scan"


def cut(T, k, m, reach=64):
    """The first streaming pattern of m bytes at or after T[k]."""
    for d in range(reach):
        P = T[k + d:k + d + m].copy()
        if len(P) == m and streaming(P):
            return P
    raise AssertionError("no streaming pattern near %d" % k)


def spread(T, m, count, lo, hi):
    """`count` streaming patterns cut from T[lo:hi) at even distances."""
    step = max(1, (hi - lo - m - 64) // count)
    return [cut(T, lo + j * step, m) for j in range(count)]


def plant(T, taken, end, P, overlap=0):
    """Copy P into T with its last byte at T[end]; the copies of a text do not overlap (but for `overlap` bytes of the last one)."""
    lo = end - len(P) + 1
    assert lo >= 0 and end < len(T) and all(hi < lo + overlap or end < a for a, hi in taken), (lo, end, taken)
    taken.append((lo, end))
    T[lo:end + 1] = P


class Case:
    """One edited text with the patterns of its group, their plans and their brute-force counts over a range (computed once)."""

    def __init__(self, po, T, pats, algos=None, off=0, n=None):
        self.T, self.pats, self.off, self.n = T, pats, off, len(T) - off if n is None else n
        self.want = [po.search("bf", P, T[off:off + self.n]) for P in pats]
        self.text = Text.upload(T)
        self.plans = [Plan(a, P) for a, P in zip(algos or ["hor"] * len(pats), pats)]
        for pl in self.plans:
            assert pl.kernel_name == "hor_scan"

    def run(self, order):
        """Launch the plans `order` (indices), one sync; -> (counts in that order, kernels sent)."""
        for pl in self.plans:
            pl.reset()
        engine.device_sync(0)
        _, p0 = engine.coalesce_stats(0)
        for j in order:
            self.plans[j].launch(self.text, off=self.off, n=self.n)
        engine.device_sync(0)
        _, p1 = engine.coalesce_stats(0)
        return [self.plans[j].result(0)[0] for j in order], p1 - p0

    def check(self, order=None):
        """One shared pass and one launch per plan give the brute-force counts."""
        order = list(range(len(self.pats)) if order is None else order)
        assert 2 <= len(order) <= 8
        want = [self.want[j] for j in order]
        engine.coalesce(8)
        got, passes = self.run(order)
        assert got == want, (len(self.T), len(self.pats[0]), order, got, want)
        assert passes == 1
        engine.coalesce(0)
        got, passes = self.run(order)
        assert got == want and passes == len(order), (len(self.T), len(self.pats[0]), order, got, want)
        engine.coalesce(8)

    def free(self):
        for pl in self.plans:
            pl.free()
        self.text.free()


# --- a window end at every offset around the tile boundaries -------------------------------------------------------
@pytest.mark.parametrize("m", (8, 18))
def test_pattern_ends_at_every_offset_around_a_tile_boundary(oracle, m):
    base = oracle.gen_text(SEED + m, 128, 0, N_BIG)
    pats = spread(base, m, 8, 100, N_BIG - 100)
    stride = 8 if m <= 8 else 32  # between the ends of two copies in one text: at least m
    for j in range(stride):
        T = base.copy()
        taken = []
        for b in (1, 2, 3):
            for r in range((j + b) % stride, 64, stride):  # over the texts, every r at every boundary
                plant(T, taken, TILE * b - 32 + r, pats[(3 * b) % 8])
        c = Case(oracle, T, pats)
        assert c.want[3] >= 64 // stride and c.want[6] >= 64 // stride and c.want[1] >= 64 // stride
        c.check()
        c.free()


# --- grams of several patterns in one slot -------------------------------------------------------------------------
def test_last_and_inner_grams_in_one_slot(oracle):
    m = 32
    T = oracle.gen_text(SEED + 256, 256, 0, N_BIG).copy()
    pats = spread(T, m, 8, 100, N_BIG - 100)
    # 37 * (a + k) + (b - 37 * k) is the same number for every k: four different grams, one slot
    a, b = 100, 200
    pats[0][m - 2:] = (a, b)
    pats[1][m - 2:] = (a + 1, b - 37)
    pats[2][5:7] = (a + 2, b - 74)
    pats[3][20:22] = (a + 3, b - 111)
    s = slot(a, b)
    assert slot(*pats[1][m - 2:]) == s and slot(*pats[2][5:7]) == s and slot(*pats[3][20:22]) == s
    assert len({tuple(pats[0][m - 2:]), tuple(pats[1][m - 2:]), tuple(pats[2][5:7]), tuple(pats[3][20:22])}) == 4
    taken = []
    for g, P in enumerate(pats):
        assert streaming(P)
        plant(T, taken, 64 * (30 + 90 * g) + 7 * g, P)
        plant(T, taken, 64 * (60 + 90 * g) + 63 - 5 * g, P)
    c = Case(oracle, T, pats)
    assert min(c.want) >= 2
    c.check()
    c.check((1, 0, 3, 2))
    c.free()


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
def test_three_patterns_with_one_last_gram(oracle, n):
    m = 17
    T = oracle.gen_text(SEED + 3, 128, 0, n).copy()
    others = spread(T, m, 5, 50, n - 50)
    A = cut(T, n // 2, m)
    variants = []  # A with another symbol at byte m - 3, still a streaming pattern
    for x in range(1, 128):
        V = A.copy()
        V[m - 3] ^= x
        if streaming(V):
            variants.append(V)
    B, C = variants[:2]
    assert len({bytes(A), bytes(B), bytes(C)}) == 3 and np.array_equal(A[m - 2:], B[m - 2:]) and np.array_equal(A[m - 2:], C[m - 2:])
    pats = others[:2] + [A] + others[2:4] + [B, C] + others[4:]
    taken = []
    for j, P in enumerate((A, B, C, B, A)):
        plant(T, taken, 64 * (9 + 11 * j) + 13 * j, P)
    c = Case(oracle, T, pats)
    assert c.want[2] >= 2 and c.want[5] >= 2 and c.want[6] >= 1
    c.check()
    c.free()


# --- lengths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
@pytest.mark.parametrize("m", (8, 17, 18, 300))
def test_lengths(oracle, n, m):
    T = oracle.gen_text(SEED + 1000 + m, 128, 0, n).copy()
    k1 = (2 * m + 63) // 64 + 1
    k2 = k1 + (m + 63) // 64 + 1
    pats = spread(T, m, 8, 64 * (k2 + 1), n - m - 10)  # cut behind the copies at the front and before the one at the end
    taken = []
    plant(T, taken, m - 1, pats[7])       # position 0
    plant(T, taken, n - 1, pats[0])       # position n - m
    plant(T, taken, 64 * k1 + 63, pats[4])  # the last window end of a lane segment
    plant(T, taken, 64 * k2, pats[4])     # the first one
    c = Case(oracle, T, pats)
    assert min(c.want) >= 1 and c.want[4] >= 2
    c.check()
    c.check((7, 0))
    c.check((4, 5, 6))
    c.free()


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
def test_length_whose_shifts_are_capped(oracle, n):
    m = CAP + 6
    T = oracle.gen_text(SEED + 2000, 128, 0, n).copy()
    pats = spread(T, m, 8, 50, n - 50)
    X = pats[2]
    X[CAP + 1:] = X[:m - CAP - 1]  # X overlaps itself CAP + 1 bytes on
    assert streaming(X)
    taken = []
    e = 64 * 20 + 10 if n == N_SMALL else TILE + 64 * 20 + 10
    plant(T, taken, e, X)
    plant(T, taken, e + CAP + 1, X, overlap=m - CAP - 1)
    plant(T, taken, e + 400, X)
    plant(T, taken, e + 400 + 2 * CAP, X)
    c = Case(oracle, T, pats)
    assert c.want[2] >= 4 and min(c.want) >= 1
    c.check()
    c.free()


# --- a range inside the text -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (8, 32, 300))
def test_range_that_starts_and_ends_inside_a_segment(oracle, m):
    T = oracle.gen_text(SEED + 3000 + m, 128, 0, N_BIG).copy()
    off, n = TILE + 616 + 21, TILE + 5000 + 10  # neither end on a 64-byte boundary; the range crosses a tile boundary
    pats = spread(T, m, 8, off + m + 10, off + n - m - 10)
    taken = []
    plant(T, taken, off + m - 1, pats[1])  # the first start position of the range
    plant(T, taken, off + n - 1, pats[6])  # the last one
    plant(T, taken, off - 1, pats[3])      # ends before the range: not counted
    plant(T, taken, off + n + m, pats[5])  # starts behind it: not counted
    c = Case(oracle, T, pats, off=off, n=n)
    whole = [oracle.search("bf", P, T) for P in pats]
    assert min(c.want) >= 1 and c.want[1] >= 2 and c.want[6] >= 2 and c.want[3] == whole[3] - 1 and c.want[5] == whole[5] - 1
    c.check()
    c.free()


# --- Tuned BM and Horspool in one group -----------------------------------------------------------------------
def test_tuned_bm_and_horspool_in_one_group(oracle):
    m = 32
    T = oracle.gen_text(SEED + 4000, 128, 0, N_BIG).copy()
    pats = [P for P in spread(T, m, 12, 100, N_BIG - 100) if streaming(P, "tunedbm")][:8]
    assert len(pats) == 8
    taken = []
    plant(T, taken, 2 * TILE, pats[1])
    plant(T, taken, 2 * TILE + 64 * 9 - 1, pats[2])
    c = Case(oracle, T, pats, algos=["hor", "tunedbm", "hor", "hor", "tunedbm", "tunedbm", "hor", "hor"])
    assert c.want[1] >= 2 and c.want[2] >= 2
    c.check()
    c.check((1, 4, 5))
    c.free()
