"""Queued Horspool launches that share one pass over the text (api.cpp's launch queue, k_horm.hip's hor_multi_scan):
every count against the oracle's brute force and against the same launches with smartgpu_coalesce(0).  Bit-exact.

Texts of 3 * 16384 + 777 bytes (four tiles, the last one partial) and of 5000 bytes (less than one tile), rand128 with
copies of the first pattern planted where the kernel has an edge: position 0 and n - m, window ends at t * 16384 - 1,
t * 16384 and t * 16384 + 15 (either side of a tile boundary, and the last byte of the 16-byte halo chunk), either side
of a 64-byte lane boundary, and — m = 18, 32 — two occurrences whose ends lie in one lane segment (the second candidate
of a lane goes through global_equal, the first through wave_verify).  m = 16, 17: the whole window is in LDS (H = 15, 16);
18: the first length completed in memory; 32: the headline; 300: a wave_verify of several steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Plan, Text, engine  # noqa: E402

TILE = 16384
N_BIG, N_SMALL = 3 * TILE + 777, 5000
MS = (16, 17, 18, 32, 300)
NPLANS = 17
SEED = 0x5EEDC0A1


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


def cut(T, k, m):
    """The first streaming pattern of m bytes at or after T[k]."""
    for d in range(64):
        P = T[k + d:k + d + m].copy()
        if streaming(P):
            return P
    raise AssertionError("no streaming pattern near %d" % k)


def planted_ends(n, m):
    """Window ends of the planted copies (see the module's docstring); the regions do not overlap for any m of MS."""
    if n == N_BIG:
        ends = [m - 1, n - 1, TILE - 1, 2 * TILE, 3 * TILE + 15, 64 * 400 - 1, 64 * 120]
        q2 = 150
    else:
        ends = [m - 1, n - 1, 64 * 40 - 1, 64 * 20]
        q2 = 50
    if m == 18:
        ends += [64 * q2 + 20, 64 * q2 + 38]
    if m == 32:
        ends += [64 * q2 + 31, 64 * q2 + 63]
    spans = sorted((e - m + 1, e) for e in ends)
    assert spans[0][0] >= 0 and spans[-1][1] < n and all(a[1] < b[0] for a, b in zip(spans, spans[1:])), spans
    return ends


class Case:
    """One edited text with its 17 patterns, their plans and their brute-force counts (computed once)."""

    def __init__(self, po, n, m):
        self.n, self.m = n, m
        T = po.gen_text(SEED + m, 128, 0, n).copy()
        P0 = cut(T, 12000 if n == N_BIG else 3500, m)
        self.ends = planted_ends(n, m)
        for e in self.ends:
            T[e - m + 1:e + 1] = P0
        self.T = T
        step = (n - m - 200) // NPLANS
        self.pats = [P0] + [cut(T, 100 + j * step, m) for j in range(1, NPLANS)]
        self.want = [po.search("bf", P, T) for P in self.pats]
        assert self.want[0] >= len(self.ends) and min(self.want) >= 1
        self.text = Text.upload(T)
        self.plans = [Plan("hor", P) for P in self.pats]
        for pl in self.plans:
            assert pl.kernel_name == "hor_scan"

    def run(self, k, **kw):
        """Launch the first k plans, one sync; -> (counts, eligible launches seen, kernels sent)."""
        for pl in self.plans:
            pl.reset()
        engine.device_sync(0)
        l0, p0 = engine.coalesce_stats(0)
        for pl in self.plans[:k]:
            pl.launch(self.text, **kw)
        engine.device_sync(0)
        l1, p1 = engine.coalesce_stats(0)
        return [pl.result(0)[0] for pl in self.plans[:k]], l1 - l0, p1 - p0


_cases = {}


@pytest.fixture
def case(oracle):
    def get(n, m):
        if (n, m) not in _cases:
            _cases[(n, m)] = Case(oracle, n, m)
        return _cases[(n, m)]
    return get


@pytest.mark.parametrize("m", MS)
def test_group_shapes(case, m):
    c = case(N_BIG, m)
    for k in (1, 2, 3, 4, 5, 8, 9, 17):
        got, launches, passes = c.run(k)
        assert got == c.want[:k], (m, k)
        assert launches == k, (m, k, launches)
        if k >= 2:
            assert passes < launches, (m, k, passes)  # the multi-pattern kernel ran
        else:
            assert passes == 1
    assert c.run(17)[2] == 3  # 8 + 8 + 1
    engine.coalesce(0)
    got, launches, passes = c.run(NPLANS)
    assert got == c.want and launches == passes == NPLANS


@pytest.mark.parametrize("m", MS)
def test_text_shorter_than_a_tile(case, m):
    c = case(N_SMALL, m)
    for k in (2, 9):
        got, launches, passes = c.run(k)
        assert got == c.want[:k] and launches == k and passes < launches, (m, k, passes)
    engine.coalesce(0)
    got, launches, passes = c.run(9)
    assert got == c.want[:9] and launches == passes == 9


@pytest.mark.parametrize("group", (2, 4))
def test_smaller_groups(case, group):
    c = case(N_BIG, 32)
    assert engine.coalesce(group) == 8
    got, launches, passes = c.run(9)
    assert got == c.want[:9] and launches == 9
    assert passes == {2: 5, 4: 3}[group]  # 2+2+2+2+1, 4+4+1
    assert engine.coalesce(8) == group


def test_same_plan_twice(case):
    c = case(N_BIG, 32)
    c.plans[0].reset()
    l0, p0 = engine.coalesce_stats(0)
    c.plans[0].launch(c.text)
    c.plans[0].launch(c.text)
    engine.device_sync(0)
    l1, p1 = engine.coalesce_stats(0)
    assert c.plans[0].result(0)[0] == 2 * c.want[0]
    assert (l1 - l0, p1 - p0) == (2, 1)


def test_two_lengths_interleaved(case, oracle):
    c = case(N_BIG, 32)
    short = [cut(c.T, 3000 + 5000 * j, 17) for j in range(3)]
    plans17 = [Plan("hor", P) for P in short]
    for pl in c.plans[:3]:
        pl.reset()
    l0, p0 = engine.coalesce_stats(0)
    for a, b in zip(c.plans[:3], plans17):
        a.launch(c.text)
        b.launch(c.text)
    engine.device_sync(0)
    l1, p1 = engine.coalesce_stats(0)
    assert [pl.result(0)[0] for pl in c.plans[:3]] == c.want[:3]
    assert [pl.result(0)[0] for pl in plans17] == [oracle.search("bf", P, c.T) for P in short]
    assert (l1 - l0, p1 - p0) == (6, 2)  # one pass per length


def test_two_ranges_interleaved(case, oracle):
    c = case(N_BIG, 32)
    inside = (TILE + 616, 5000)  # starts and ends inside the second tile
    whole = (0, c.n)
    for pl in c.plans[:6]:
        pl.reset()
    l0, p0 = engine.coalesce_stats(0)
    for j in range(3):
        c.plans[2 * j].launch(c.text, off=whole[0], n=whole[1])
        c.plans[2 * j + 1].launch(c.text, off=inside[0], n=inside[1])
    # ... and the planted pattern over a range that cuts its copy at the tile boundary: slot 1
    cutting = (TILE - 20, 2 * TILE + 100)
    c.plans[0].launch(c.text, slot=1, off=cutting[0], n=cutting[1])
    c.plans[1].launch(c.text, slot=1, off=cutting[0], n=cutting[1])
    engine.device_sync(0)
    l1, p1 = engine.coalesce_stats(0)
    for j in range(3):
        assert c.plans[2 * j].result(0)[0] == c.want[2 * j]
        P = c.pats[2 * j + 1]
        assert c.plans[2 * j + 1].result(0)[0] == oracle.search("bf", P, c.T[inside[0]:inside[0] + inside[1]])
    for j in range(2):
        assert c.plans[j].result(1)[0] == oracle.search("bf", c.pats[j], c.T[cutting[0]:cutting[0] + cutting[1]])
    assert (l1 - l0, p1 - p0) == (8, 3)


def test_other_kernel_between(case):
    c = case(N_BIG, 32)
    kmp = Plan("kmp", c.pats[0])
    for pl in c.plans[:4]:
        pl.reset()
    c.plans[0].launch(c.text)
    c.plans[1].launch(c.text)
    kmp.launch(c.text)  # sends the two before it
    c.plans[2].launch(c.text)
    c.plans[3].launch(c.text)
    engine.device_sync(0)
    assert kmp.result(0)[0] == c.want[0]
    assert [pl.result(0)[0] for pl in c.plans[:4]] == c.want[:4]


def test_reset_between_launches(case):
    c = case(N_BIG, 32)
    c.plans[0].reset()
    c.plans[1].reset()
    c.plans[0].launch(c.text)
    c.plans[1].launch(c.text)
    c.plans[0].reset()  # after the launch before it: that count is gone
    c.plans[0].launch(c.text)
    c.plans[1].launch(c.text)
    assert c.plans[0].result(0)[0] == c.want[0]
    assert c.plans[1].result(0)[0] == 2 * c.want[1]


def test_timed_launch_in_the_middle(case):
    c = case(N_BIG, 32)
    for pl in c.plans[:5]:
        pl.reset()
    l0, p0 = engine.coalesce_stats(0)
    c.plans[0].launch(c.text)
    c.plans[1].launch(c.text)
    c.plans[2].launch(c.text, timed=True)
    c.plans[3].launch(c.text)
    c.plans[4].launch(c.text)
    got = [pl.result(0) for pl in c.plans[:5]]
    l1, p1 = engine.coalesce_stats(0)
    assert [g[0] for g in got] == c.want[:5]
    assert got[2][1] > 0 and all(got[j][1] == -1.0 for j in (0, 1, 3, 4))
    assert (l1 - l0, p1 - p0) == (5, 3)


def test_free_with_launches_pending(case, oracle):
    c = case(N_BIG, 32)
    doomed = Plan("hor", c.pats[5])
    for pl in c.plans[:2]:
        pl.reset()
    c.plans[0].launch(c.text)
    doomed.launch(c.text)
    c.plans[1].launch(c.text)
    doomed.free()  # sends what is pending, then frees
    assert [pl.result(0)[0] for pl in c.plans[:2]] == c.want[:2]
    # a text freed with launches over it pending
    T2 = c.T[:N_SMALL + 123].copy()
    text2 = Text.upload(T2)
    ps = [Plan("hor", P) for P in c.pats[:3]]
    c.plans[2].reset()
    for pl in ps:
        pl.launch(text2)
    c.plans[2].launch(c.text)
    text2.free()
    assert [pl.result(0)[0] for pl in ps] == [oracle.search("bf", P, T2) for P in c.pats[:3]]
    assert c.plans[2].result(0)[0] == c.want[2]


def test_external_result_buffer(case):
    c = case(N_BIG, 32)
    holder = Plan("hor", c.pats[0])  # its 4096 zeroed result slots serve as the caller's device buffer
    base = holder.result_device_ptr
    mine = [Plan("hor", P) for P in c.pats[:3]]
    for j, pl in enumerate(mine):
        pl.set_result_buffer(base + 8 * (10 + j), 1)
        pl.launch(c.text)
    mine[0].set_result_buffer(base + 8 * 20, 1)  # the launch before it counts into the buffer it was given
    mine[0].launch(c.text)
    engine.device_sync(0)
    assert [holder.result(10 + j)[0] for j in range(3)] == c.want[:3]
    assert holder.result(20)[0] == c.want[0]
    for pl in mine:
        pl.set_result_buffer(None, 0)


def test_tuned_bm_shares_a_pass_with_horspool(case):
    c = case(N_BIG, 32)
    tbm = Plan("tunedbm", c.pats[1])
    assert tbm.kernel_name == "hor_scan"
    c.plans[0].reset()
    l0, p0 = engine.coalesce_stats(0)
    c.plans[0].launch(c.text)
    tbm.launch(c.text)
    engine.device_sync(0)
    l1, p1 = engine.coalesce_stats(0)
    assert (c.plans[0].result(0)[0], tbm.result(0)[0]) == (c.want[0], c.want[1])
    assert (l1 - l0, p1 - p0) == (2, 1)
