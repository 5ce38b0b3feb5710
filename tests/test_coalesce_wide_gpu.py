"""Shared passes of up to 32 launches (smartgpu_coalesce_wide; k_horm.hip: a skip-table entry's eight bits are CLASSES,
pattern g sets bit g & 7, and a window that ends in a class's gram is compared with every pattern of the class).  What
the wider pass can get wrong, at m = 8, 17 (m - 1 = H), 32 and 100 (windows completed in memory):

* groups of 9, 15, 16, 17, 24, 31, 32, 33 and 65 launches: 33 make two kernels, 65 three, and 32 that have gathered are
  sent before anything waits;
* the LAST pattern of a group of 32 at position 0 and at n - m;
* copies of patterns 3 and 11 (one class, and the same last gram) and of 5 and 6 (two classes) that end in one 64-byte
  lane segment: the first segment of a tile, where the earlier copy is compared in the halo, the last one, one inside;
* patterns 14 and 22 (one class) with different last grams that share a table slot;
* identical patterns in slots 2 and 10 and in slots 7 and 31: both slots get the whole count;
* m = 100: patterns 20 and 28 (one class) overlap by 70 bytes, so their copies end 30 bytes apart in ONE lane — the first
  candidate is parked for the wave-wide compare, the second is completed by its lane — and a third copy in the same wave;
* a Tuned BM plan among Horspool plans, a sub-range that starts inside a tile;
* smartgpu_coalesce(8), the old call: 17 launches make three kernels.

Every count against the oracle's brute force and against the same launches under smartgpu_coalesce(0).  Bit-exact.
Texts of 3 * 16384 + 777 and of 5000 bytes.  The helpers are those of tests/test_coalesce_gram_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from smart_amd import engine  # noqa: E402
from test_coalesce_gram_gpu import N_BIG, N_SMALL, TILE, Case, cut, need_gpu, plant, spread, streaming  # noqa: E402,F401

SEED = 0x5EED0320
MS = (8, 17, 32, 100)
GROUPS = (9, 15, 16, 17, 24, 31, 32, 33, 65)
NPATS = 65
WIDTH = 32


@pytest.fixture(autouse=True)
def groups_of_thirty_two():
    """Every test starts with passes of up to 32 launches, set through the new call, and leaves behind what it found."""
    found = engine.coalesce_wide(WIDTH)
    yield
    engine.device_sync(0)
    engine.coalesce_wide(found)


def edited_patterns(po, m, n, salt):
    fresh = po.gen_text(SEED + 7 * m + 1000 * salt, 128, 0, n)  # bytes that patterns are cut from, whatever is planted into T
    pats = spread(fresh, m, NPATS, 100, n - 100)
    assert len({bytes(P) for P in pats}) == NPATS
    pats[11][m - 2:] = pats[3][m - 2:]  # class mates that survive their last gram
    pats[14][m - 2:] = (10, 20)   # 37 * 10 + 20 and 37 * 120 + 46 differ by 4096: two last grams of one class in one slot
    pats[22][m - 2:] = (120, 46)
    pats[10] = pats[2].copy()
    pats[31] = pats[7].copy()
    if m == 100:
        pats[28] = np.concatenate([pats[20][30:], pats[28][:30]])  # pats[20] ending at e, pats[28] at e + 30: both whole
    return pats


def edited(po, m, n):
    """-> (T, pats): a rand128 text of n bytes and NPATS streaming patterns of m bytes with the copies the module's
    docstring lists (the big text has them all; the small one the copies at both ends and the identical patterns)."""
    T = po.gen_text(SEED + m, 128, 0, n).copy()
    for salt in range(16):  # (nearly always the first: an edited pattern may repeat its symbols)
        pats = edited_patterns(po, m, n, salt)
        if all(streaming(P) for P in pats):
            break
    else:
        raise AssertionError("no %d streaming patterns: m %d n %d" % (NPATS, m, n))
    taken = []
    plant(T, taken, m - 1, pats[31])  # position 0
    plant(T, taken, n - 1, pats[31])  # position n - m
    if n == N_BIG:
        if m < 64:
            for b, (g, h) in ((1, (3, 11)), (3, (5, 6))):
                plant(T, taken, TILE * b + 3, pats[g])   # the window lies in the halo but for four bytes
                plant(T, taken, TILE * b + 40, pats[h])  # ... and the same lane meets this one
            plant(T, taken, 2 * TILE - 64 + 3, pats[11])
            plant(T, taken, 2 * TILE - 1, pats[3])       # the tile's last window end
            plant(T, taken, 2 * TILE + 64 * 50 + 3, pats[6])
            plant(T, taken, 2 * TILE + 64 * 50 + 40, pats[5])
        else:
            for e in (TILE + 64 * 9 + 10, 2 * TILE + 3):  # inside a tile; the first lane of a tile
                plant(T, taken, e, pats[20])
                plant(T, taken, e + 30, pats[28], overlap=m - 30)
            plant(T, taken, TILE + 64 * 12 + 50, pats[20])  # a third candidate of the class in the wave of the first two
    big = n == N_BIG
    elsewhere = {7, 31} | ({3, 11, 5, 6} if big and m < 64 else set()) | ({20, 28} if big and m >= 64 else set())
    stride = 192 if big else 64 if m <= 32 else 128
    for j, P in enumerate(pats):  # every other pattern once, as far as the text has room, away from the copies above
        end = 64 * 4 + stride * j + 2 * m
        if j not in elsewhere and end < min(n - 2 * m, TILE - 2 * m):
            plant(T, taken, end, P)
    return T, pats


_cases = {}


@pytest.fixture
def case(oracle):
    def get(n, m):
        if (n, m) not in _cases:
            _cases[(n, m)] = Case(oracle, *edited(oracle, m, n))
        return _cases[(n, m)]
    return get


def passes_of(k, width=WIDTH):
    return -(-k // width)  # a launch that is alone at the end is a kernel all the same


@pytest.mark.parametrize("m", MS)
def test_group_sizes(case, m):
    c = case(N_BIG, m)
    assert c.want[31] >= 2 and c.want[2] == c.want[10] >= 1 and c.want[7] == c.want[31]
    if m < 64:
        assert min(c.want[g] for g in (3, 11, 5, 6)) >= 2
    else:
        assert c.want[20] >= 3 and c.want[28] >= 2
    for k in GROUPS:
        got, passes = c.run(range(k))
        assert got == c.want[:k], (m, k)
        assert passes == passes_of(k), (m, k, passes)
    # another order: the patterns change their slots and their classes
    order = list(range(NPATS - 1, -1, -1))[:WIDTH + 5]
    got, passes = c.run(order)
    assert got == [c.want[j] for j in order] and passes == 2, m
    engine.coalesce(0)
    got, passes = c.run(range(NPATS))
    assert got == c.want and passes == NPATS, m


@pytest.mark.parametrize("m", MS)
def test_text_shorter_than_a_tile(case, m):
    c = case(N_SMALL, m)
    assert c.want[31] >= 2 and c.want[2] == c.want[10] and c.want[7] == c.want[31]
    for k in (9, 32, 33):
        got, passes = c.run(range(k))
        assert got == c.want[:k] and passes == passes_of(k), (m, k, passes)
    engine.coalesce(0)
    got, passes = c.run(range(33))
    assert got == c.want[:33] and passes == 33, m


@pytest.mark.parametrize("m", (17, 100))
def test_thirty_two_gathered_are_sent_before_anything_waits(case, m):
    c = case(N_BIG, m)
    for pl in c.plans:
        pl.reset()
    engine.device_sync(0)
    l0, p0 = engine.coalesce_stats(0)
    for pl in c.plans[:31]:
        pl.launch(c.text)
    assert engine.coalesce_stats(0)[1] - p0 == 0  # 31 are gathering
    c.plans[31].launch(c.text)
    assert engine.coalesce_stats(0)[1] - p0 == 1  # the 32nd sent them
    c.plans[32].launch(c.text)
    l1, p1 = engine.coalesce_stats(0)
    assert (l1 - l0, p1 - p0) == (33, 1)  # one is pending
    assert [pl.result(0)[0] for pl in c.plans[:33]] == c.want[:33]
    assert engine.coalesce_stats(0)[1] - p0 == 2


def test_a_tuned_bm_plan_among_horspool_plans(oracle):
    m = 32
    T = oracle.gen_text(SEED + 4000, 128, 0, N_BIG).copy()
    pats = [P for P in spread(T, m, 40, 100, N_BIG - 100) if streaming(P, "tunedbm")][:WIDTH]
    assert len(pats) == WIDTH
    taken = []
    plant(T, taken, 2 * TILE, pats[9])
    plant(T, taken, 2 * TILE + 64 * 9 - 1, pats[17])
    algos = ["tunedbm" if j in (1, 9, 30) else "hor" for j in range(WIDTH)]
    c = Case(oracle, T, pats, algos=algos)
    assert c.want[9] >= 2 and c.want[17] >= 2 and min(c.want) >= 1
    got, passes = c.run(range(WIDTH))
    assert got == c.want and passes == 1
    engine.coalesce(0)
    got, passes = c.run(range(WIDTH))
    assert got == c.want and passes == WIDTH
    c.free()


@pytest.mark.parametrize("m", (8, 32, 100))
def test_a_range_that_starts_inside_a_tile(oracle, m):
    T = oracle.gen_text(SEED + 3000 + m, 128, 0, N_BIG).copy()
    off, n = TILE + 616 + 21, TILE + 5000 + 10  # neither end on a 64-byte boundary; the range crosses a tile boundary
    pats = spread(T, m, WIDTH, off + m + 10, off + n - m - 10)
    taken = []
    plant(T, taken, off + m - 1, pats[9])   # the first start position of the range
    plant(T, taken, off + n - 1, pats[31])  # the last one
    plant(T, taken, off - 1, pats[3])       # ends before the range: not counted
    plant(T, taken, off + n + m, pats[29])  # starts behind it: not counted
    c = Case(oracle, T, pats, off=off, n=n)
    whole = [oracle.search("bf", P, T) for P in pats]
    assert min(c.want) >= 1 and c.want[9] >= 2 and c.want[31] >= 2 and c.want[3] == whole[3] - 1 and c.want[29] == whole[29] - 1
    got, passes = c.run(range(WIDTH))
    assert got == c.want and passes == 1, m
    engine.coalesce(0)
    got, passes = c.run(range(WIDTH))
    assert got == c.want and passes == WIDTH, m
    c.free()


def test_the_old_call_still_makes_passes_of_eight(case):
    c = case(N_BIG, 32)
    assert engine.coalesce(8) == 8  # the old call reports the width of 32 as 8
    got, passes = c.run(range(17))
    assert got == c.want[:17] and passes == 3  # 8 + 8 + 1
    assert engine.coalesce_wide(WIDTH) == 8
