"""Shared passes of up to 96 launches (smartgpu_coalesce_pass; k_horm.hip: a byte skip table of 16384 slots, a hit bit,
and per gram bucket a chain of the patterns whose last gram falls into it).  What the wider pass can get wrong:

* groups of 33, 64, 83, 84, 85, 96, 97 and 200 launches at m = 8, 17 and 18 (either side of the halo), 32, 64 and 65
  (either side of the row stride) and 100 (windows completed in memory): a pass takes engine.pass_width(m) launches at
  the most, whatever the setting, so k launches make ceil(k / width) kernels (no key is sent before it is full or
  something waits; the bounds ceil(k / width) <= kernels <= ceil(k / 32) + 1 hold with it);
* patterns 3 and 11 with one last gram; patterns 14 and 22 with different last grams in one bucket; the same pattern in
  slots 2 and 10; pattern 5's last gram as an inner gram of pattern 6; the pass's last pattern at position 0 and n - m;
* m = 100: patterns 20 and 28 overlap by 70 bytes, so their copies end 30 bytes apart in ONE lane — the first
  candidate is parked for the wave-wide compare, the second is completed by its lane — and a third copy in that wave;
* texts of 8 MiB with one workgroup per CU (smartgpu_tune(4, 1)): a workgroup walks more than one tile with one table;
* a range that begins and ends inside a tile; a text with byte values of 128 and more (slots alias there);
* launches of other algorithms between the queued ones.

Every count against the oracle's brute force and against the same launches under smartgpu_coalesce(0).  Bit-exact.
The helpers are those of tests/test_coalesce_gram_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from smart_amd import Plan, engine  # noqa: E402
from test_coalesce_gram_gpu import TILE, Case, need_gpu, plant, spread, streaming  # noqa: E402,F401

SEED = 0x5EED0960
N = 8 << 20
MS = (8, 17, 18, 32, 64, 65, 100)
GROUPS = (33, 64, 83, 84, 85, 96, 97, 200)
NPATS = 200
NARROW = 32


def gram_slot(prev, last):
    """multi.hpp gram_slot"""
    return (128 * int(prev) + 85 * (int(prev) >> 7) + int(last)) & 16383


def gram_bucket(prev, last):
    """multi.hpp gram_bucket"""
    return ((gram_slot(prev, last) * 0x9E3779B1) & 0xFFFFFFFF) >> 23


@pytest.fixture(autouse=True)
def widest_passes_one_workgroup_per_cu():
    """Every test starts with the widest passes and one workgroup per CU, and leaves behind what it found."""
    found = engine.coalesce_pass(engine.PASS_MAX)
    engine.tune(4, 1)
    yield
    engine.device_sync(0)
    engine.tune(4, 0)
    engine.coalesce_pass(found)


def edited_patterns(po, m, n, sigma, salt):
    fresh = po.gen_text(SEED + 7 * m + 1000 * salt + sigma, sigma, 0, n)  # bytes that patterns are cut from, whatever is planted into T
    pats = spread(fresh, m, NPATS, 100, n - 100)
    assert len({bytes(P) for P in pats}) == NPATS
    pats[11][m - 2:] = pats[3][m - 2:]      # one last gram, two patterns
    a, b = (int(x) for x in pats[14][m - 2:])
    mates = [(c, d) for c in range(sigma) for d in range(sigma) if gram_bucket(c, d) == gram_bucket(a, b) and gram_slot(c, d) != gram_slot(a, b)]
    pats[22][m - 2:] = mates[salt % len(mates)]  # one bucket, two last grams
    pats[10] = pats[2].copy()                # one pattern, two slots
    pats[6][m - 5:m - 3] = pats[5][m - 2:]   # the last gram of 5 inside 6
    if m == 100:
        pats[28] = np.concatenate([pats[20][30:], pats[28][:30]])  # pats[20] ending at e, pats[28] at e + 30: both whole
    return pats


def edited(po, m, n, sigma):
    """-> (T, pats): a text of n bytes over `sigma` symbols and NPATS streaming patterns of m bytes with the copies the
    module's docstring lists."""
    T = po.gen_text(SEED + m + sigma, sigma, 0, n).copy()
    for salt in range(16):  # (nearly always the first: an edited pattern may repeat its symbols)
        pats = edited_patterns(po, m, n, sigma, salt)
        if all(streaming(P) for P in pats):
            break
    else:
        raise AssertionError("no %d streaming patterns: m %d n %d" % (NPATS, m, n))
    taken = []
    plant(T, taken, m - 1, pats[32])  # position 0: the last pattern of a first pass of 33
    plant(T, taken, n - 1, pats[32])  # position n - m
    if m == 100:
        for e in (TILE + 64 * 9 + 10, 300 * TILE + 3):  # inside a tile; the first lane of a tile a workgroup reaches second
            plant(T, taken, e, pats[20])
            plant(T, taken, e + 30, pats[28], overlap=m - 30)
        plant(T, taken, TILE + 64 * 12 + 50, pats[20])  # a third candidate in the wave of the first two
    else:
        plant(T, taken, 300 * TILE + 3, pats[3])    # the window lies in the halo but for four bytes; a workgroup's second tile
        plant(T, taken, 300 * TILE + 3 + m, pats[11])  # ... and the same lane, or its neighbour, meets this one
    for j, g in enumerate((14, 22, 2, 5, 6, 83, 84, 95, 96, 199)):
        plant(T, taken, 2 * TILE + 64 * 7 * (j + 1) + 5 * j + 2 * m, pats[g])
    for j, P in enumerate(pats):  # every pattern once more, away from the copies above
        plant(T, taken, 3 * TILE + 64 * 5 * j + 3 * j + 2 * m, P)
    return T, pats


_texts, _cases = {}, {}


@pytest.fixture
def case(oracle):
    def get(m, sigma=128, off=0, n=None, npats=NPATS):
        key = (m, sigma, off, n, npats)
        if key not in _cases:
            if (m, sigma) not in _texts:
                _texts[(m, sigma)] = edited(oracle, m, N, sigma)
            T, pats = _texts[(m, sigma)]
            _cases[key] = Case(oracle, T, pats[:npats], off=off, n=n)
        return _cases[key]
    return get


def check_group(c, m, order):
    """The launches `order` under the widest passes: counts, and the kernels they took."""
    k, width = len(order), engine.pass_width(m)
    got, passes = c.run(order)
    assert got == [c.want[j] for j in order], (m, k)
    assert -(-k // width) <= passes <= -(-k // NARROW) + 1, (m, k, passes)
    assert passes == -(-k // width), (m, k, passes)


@pytest.mark.parametrize("m", MS)
def test_group_sizes(case, m):
    c = case(m)
    assert c.want[32] >= 2 and c.want[2] == c.want[10] >= 1 and min(c.want[g] for g in (3, 11, 14, 22, 5, 6)) >= 1
    if m == 100:
        assert c.want[20] >= 3 and c.want[28] >= 2
    for k in GROUPS:
        check_group(c, m, range(k))
    # another order: the patterns change their slots and their places on the chains
    check_group(c, m, list(range(engine.pass_width(m) + 4, -1, -1)))
    # a width of 32 through the older call: exactly ceil(k / 32) kernels
    assert engine.coalesce_wide(NARROW) == NARROW  # (the widest setting, reported as 32)
    for k in (33, 97):
        got, passes = c.run(range(k))
        assert got == c.want[:k] and passes == -(-k // NARROW), (m, k, passes)
    engine.coalesce(0)
    got, passes = c.run(range(NPATS))
    assert got == c.want and passes == NPATS, m


@pytest.mark.parametrize("m", (17, 65))
def test_a_full_key_is_sent_before_anything_waits(case, m):
    c = case(m)
    width = engine.pass_width(m)
    for pl in c.plans:
        pl.reset()
    engine.device_sync(0)
    _, p0 = engine.coalesce_stats(0)
    for pl in c.plans[:width - 1]:
        pl.launch(c.text)
    assert engine.coalesce_stats(0)[1] - p0 == 0  # width - 1 are gathering
    c.plans[width - 1].launch(c.text)
    assert engine.coalesce_stats(0)[1] - p0 == 1  # the key was full just now
    c.plans[width].launch(c.text)
    assert engine.coalesce_stats(0)[1] - p0 == 1  # one is pending
    assert [pl.result(0)[0] for pl in c.plans[:width + 1]] == c.want[:width + 1]
    assert engine.coalesce_stats(0)[1] - p0 == 2


@pytest.mark.parametrize("m", (8, 32, 100))
def test_a_range_that_begins_and_ends_inside_a_tile(oracle, case, m):
    off, n = 2 * TILE + 616 + 21, 300 * TILE + 5000 + 10  # neither end on a 64-byte boundary
    c = case(m, off=off, n=n, npats=97)
    whole = case(m)
    assert c.want[32] == whole.want[32] - 2 and sum(c.want) < sum(whole.want) and min(c.want[g] for g in (14, 22, 2, 5, 6, 83, 84)) >= 1
    for k in (84, 97):
        check_group(c, m, range(k))
    engine.coalesce(0)
    got, passes = c.run(range(97))
    assert got == c.want[:97] and passes == 97, m


@pytest.mark.parametrize("m", (17, 32))
def test_byte_values_of_128_and_more(case, m):
    c = case(m, sigma=256, npats=97)
    assert max(int(P.max()) for P in c.pats) >= 128 and min(c.want) >= 1
    for k in (84, 85, 97):
        check_group(c, m, range(k))
    engine.coalesce(0)
    got, passes = c.run(range(97))
    assert got == c.want and passes == 97, m


@pytest.mark.parametrize("m", (32, 100))
def test_launches_of_other_algorithms_between_the_queued_ones(oracle, case, m):
    c = case(m)
    others = [Plan("kmp", c.pats[0]), Plan("bm", c.pats[1])]
    try:
        for pl in c.plans + others:
            pl.reset()
        engine.device_sync(0)
        l0, p0 = engine.coalesce_stats(0)
        for j, pl in enumerate(c.plans[:97]):
            pl.launch(c.text)
            if j % 10 == 5:
                others[(j // 10) % 2].launch(c.text)
        engine.device_sync(0)
        l1, p1 = engine.coalesce_stats(0)
        assert [pl.result(0)[0] for pl in c.plans[:97]] == c.want[:97], m
        assert [pl.result(0)[0] for pl in others] == [5 * c.want[0], 5 * c.want[1]], m
        assert l1 - l0 == 97 and p1 - p0 == -(-97 // engine.pass_width(m))
    finally:
        for pl in others:
            pl.free()
