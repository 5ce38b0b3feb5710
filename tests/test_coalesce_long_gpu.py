"""Long passes of hor_multi_scan on the device (k_horm.hip; api.cpp: the queue's gathering rule; smartgpu_coalesce_long).
A key whose previous pass left because it was full goes on gathering beyond pass_width(m), up to long_width(m), and is
sent as ONE kernel that carries pointers only and reads its rows from the plans' blobs.  What that can get wrong:

* the rows: 16-byte pieces read from blob + gram_first(m) + offset, two pieces per thread where np rows are more than
  256 pieces (m = 32: 304; 33: 324; 65, 100: 340), at no alignment for m = 100 (gram_first = 35);
* links and sums of np entries behind the rows, at offsets that follow np: k launches with W = pass_width(m) and
  LW = long_width(m) for k = W, W + 1, W + LW - 1, W + LW, W + LW + 1 and 270 give one pass of W and long passes of
  1 (a solo scan), LW - 1, LW, LW and 1, and what is left; in reversed order the patterns change slots, chains and threads;
* exactly 1 + ceil((k - W) / LW) kernels for k > W and 1 for k <= W;
* m = 8, 16 (252 patterns), 17 (H = m - 1), 32, 33, 65 and 100 (windows completed in memory from the long layout's blob);
* the same plan twice in one long pass; a rider in a long pass, which takes a place; a pattern planted as a periodic run
  of 40 copies across a tile boundary at a place g >= W; the pattern at the last place, LW - 1, at text positions 0 and n - m;
* a range that begins and ends inside a tile; byte values of 128 and more (sigma 256: the folded slots);
* after a flush the next pass leaves at W again; with the default threshold (64 MiB) and with -1 the same 8 MiB
  launches make ceil(k / W) passes.

Texts of 8 MiB with one workgroup per CU (smartgpu_tune(4, 1)): every workgroup walks two tiles with one table and the
prefetch runs.  270 patterns, planted once each; where k exceeds 270 the launches go round (a plan's counts add up).
Every count against the oracle's brute force.  Bit-exact.  All inputs are valid searches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from smart_amd import Plan, engine  # noqa: E402
from test_coalesce_gram_gpu import TILE, Case, need_gpu, plant, spread, streaming  # noqa: E402,F401
from test_coalesce_ride_gpu import can_ride, repeating  # noqa: E402

SEED = 0x5EED1096
N = 8 << 20
MS = (8, 16, 17, 32, 33, 65, 100)
NPATS = 270
RUN = 40  # copies in the periodic run
RIDER_MS = (32, 100)


@pytest.fixture(autouse=True)
def long_passes_over_any_range_one_workgroup_per_cu():
    """Every test starts with the widest passes, long passes over any range and one workgroup per CU, and leaves behind
    what it found."""
    width = engine.coalesce_pass(engine.PASS_MAX)
    least = engine.coalesce_long(0)
    engine.tune(4, 1)
    try:
        yield
    finally:
        engine.device_sync(0)
        engine.tune(4, 0)
        engine.coalesce_long(least)
        engine.coalesce_pass(width)


def frequent(m):
    """the plan whose pattern is planted as a periodic run: at place W + 3 of a region's launches, in the first long pass"""
    return engine.pass_width(m) + 3


def last_place(m):
    """the plan at the last place of the first long pass"""
    return (engine.pass_width(m) + engine.long_width(m) - 1) % NPATS


def edited(po, m, sigma):
    T = po.gen_text(SEED + m + sigma, sigma, 0, N).copy()
    fresh = po.gen_text(SEED + 7 * m + sigma, sigma, 0, N)
    pats = spread(fresh, m, NPATS, 100, N - 100)
    assert len({bytes(P) for P in pats}) == NPATS and all(streaming(P) for P in pats)
    taken = []
    plant(T, taken, m - 1, pats[last_place(m)])  # position 0
    plant(T, taken, N - 1, pats[last_place(m)])  # position n - m
    for j, P in enumerate(pats):
        plant(T, taken, 3 * TILE + 64 * 5 * j + 3 * j + 2 * m, P)
    for r in range(RUN):  # 20 copies on either side of a tile boundary, in a tile that a workgroup reaches second
        plant(T, taken, 300 * TILE - (RUN // 2 - r) * m + m - 1, pats[frequent(m)])
    if m in RIDER_MS:
        for at in (1000, 5000, 9000):
            plant(T, taken, 200 * TILE + at, rider(T, m))
    return T, pats


def rider(T, m):
    """A pattern whose own symbols repeat, from bytes of T that nothing is planted into."""
    return repeating(T, m, at=150 * TILE + 1000)


_texts, _cases = {}, {}


@pytest.fixture
def case(oracle):
    def get(m, sigma=128, off=0, n=None):
        key = (m, sigma, off, n)
        if key not in _cases:
            if (m, sigma) not in _texts:
                _texts[(m, sigma)] = edited(oracle, m, sigma)
            T, pats = _texts[(m, sigma)]
            _cases[key] = Case(oracle, T, pats, off=off, n=n)
        return _cases[key]
    return get


def launch_all(c, order):
    """Launch the plans `order` in one region; -> kernels sent.  Every plan's count must be the oracle's, times its launches."""
    for pl in c.plans:
        pl.reset()
    engine.device_sync(0)
    _, p0 = engine.coalesce_stats(0)
    times = [0] * len(c.plans)
    for j in order:
        c.plans[j].launch(c.text, off=c.off, n=c.n)
        times[j] += 1
    engine.device_sync(0)
    _, p1 = engine.coalesce_stats(0)
    got = [pl.result(0)[0] for pl in c.plans]
    want = [w * t for w, t in zip(c.want, times)]
    wrong = [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, (len(c.pats[0]), len(order), wrong[:8])
    return p1 - p0


def expected_passes(m, k):
    W, LW = engine.pass_width(m), engine.long_width(m)
    return 1 if k <= W else 1 + -(-(k - W) // LW)


def group_sizes(m):
    W, LW = engine.pass_width(m), engine.long_width(m)
    return (W, W + 1, W + LW - 1, W + LW, W + LW + 1, NPATS)


def check_sizes(c, m):
    for k in group_sizes(m):
        assert launch_all(c, [j % NPATS for j in range(k)]) == expected_passes(m, k), (m, k)
        # reversed: the patterns change their slots, their places on the chains and the threads that read their rows
        assert launch_all(c, [j % NPATS for j in range(k - 1, -1, -1)]) == expected_passes(m, k), (m, k, "reversed")


@pytest.mark.parametrize("m", MS)
def test_group_sizes(case, m):
    c = case(m)
    assert c.want[frequent(m)] >= RUN + 1 and c.want[last_place(m)] >= 3 and min(c.want) >= 1
    assert engine.long_width(m) > engine.pass_width(m)
    check_sizes(c, m)


@pytest.mark.parametrize("m", (16, 32, 100))
def test_byte_values_of_128_and_more(case, m):
    c = case(m, sigma=256)
    assert max(int(P.max()) for P in c.pats) >= 128 and min(c.want) >= 1 and c.want[frequent(m)] >= RUN + 1
    check_sizes(c, m)


@pytest.mark.parametrize("m", (32, 100))
def test_a_range_that_begins_and_ends_inside_a_tile(case, m):
    off, n = 2 * TILE + 616 + 21, 300 * TILE + 5000 + 10  # neither end on a 64-byte boundary; the run lies inside
    c, whole = case(m, off=off, n=n), case(m)
    # (the copies at positions 0 and n - m lie outside the range)
    assert 1 <= c.want[last_place(m)] <= whole.want[last_place(m)] - 2 and c.want[frequent(m)] >= RUN + 1 and min(c.want) >= 1
    W, LW = engine.pass_width(m), engine.long_width(m)
    for k in (W + LW, NPATS):
        assert launch_all(c, list(range(k))) == expected_passes(m, k), (m, k)


@pytest.mark.parametrize("m", (17, 32, 100))
def test_the_same_plan_twice_in_one_long_pass(case, m):
    c = case(m)
    W, LW = engine.pass_width(m), engine.long_width(m)
    order = list(range(W + LW))
    order[W + 1] = order[W + LW - 1] = frequent(m)  # three times in the long pass: places 1, 3 and LW - 1
    order[W + 7] = 2                                # once in the pass of W, once in the long one
    assert launch_all(c, order) == 2, m


@pytest.mark.parametrize("m", RIDER_MS)
def test_a_rider_in_a_long_pass(oracle, case, m):
    c = case(m)
    W, LW = engine.pass_width(m), engine.long_width(m)
    R = rider(c.T, m)  # planted three times (edited)
    assert can_ride(R)
    want_r = oracle.search("bf", R, c.T)
    assert want_r >= 3 and c.text.repeat_rate() * 48 <= 1
    rplan = Plan("hor", R)
    try:
        for pl in c.plans:
            pl.reset()
        engine.device_sync(0)
        _, p0 = engine.coalesce_stats(0)
        r0 = engine.coalesce_riders(0)
        for j in range(W + 5):
            c.plans[j].launch(c.text)
        assert engine.coalesce_stats(0)[1] - p0 == 1  # the pass of W left; five are gathering
        rplan.launch(c.text)                          # place 5 of the long pass
        for j in range(W + 5, W + LW - 2):
            c.plans[j % NPATS].launch(c.text)
        assert engine.coalesce_stats(0)[1] - p0 == 1  # LW - 1 entries, one of them the rider
        rplan.launch(c.text)                          # the rider takes the last place and the key is full
        assert engine.coalesce_stats(0)[1] - p0 == 2 and engine.coalesce_riders(0) - r0 == 2
        engine.device_sync(0)
        assert engine.coalesce_stats(0)[1] - p0 == 2
        assert rplan.result(0)[0] == 2 * want_r, (m, want_r)
        times = [0] * NPATS
        for j in range(W + LW - 2):
            times[j % NPATS] += 1
        assert [pl.result(0)[0] for pl in c.plans] == [w * t for w, t in zip(c.want, times)], m
    finally:
        engine.device_sync(0)
        rplan.free()


def test_after_a_flush_the_next_pass_leaves_at_the_by_value_width_again(case):
    m = 32
    c = case(m)
    W, LW = engine.pass_width(m), engine.long_width(m)
    for pl in c.plans:
        pl.reset()
    engine.device_sync(0)
    _, p0 = engine.coalesce_stats(0)
    sent = lambda: engine.coalesce_stats(0)[1] - p0  # noqa: E731
    for j in range(W - 1):
        c.plans[j].launch(c.text)
    assert sent() == 0
    c.plans[W - 1].launch(c.text)
    assert sent() == 1  # full at W: nothing was sent before it
    for j in range(W, W + LW - 1):
        c.plans[j % NPATS].launch(c.text)
    assert sent() == 1  # LW - 1 are gathering, more than W
    engine.device_sync(0)
    assert sent() == 2  # the flush sent them, as one long pass
    for j in range(W):
        c.plans[j].launch(c.text)
    assert sent() == 3  # after the flush a pass leaves at W again
    for j in range(W, W + LW):
        c.plans[j % NPATS].launch(c.text)
    assert sent() == 4  # ... and the one behind it at LW
    engine.device_sync(0)
    assert sent() == 4
    times = [0] * NPATS
    for j in list(range(W + LW - 1)) + list(range(W + LW)):
        times[j % NPATS] += 1
    assert [pl.result(0)[0] for pl in c.plans] == [w * t for w, t in zip(c.want, times)]


@pytest.mark.parametrize("least", (engine.LONG_DEFAULT, -1, N))
def test_below_the_threshold_and_switched_off_a_pass_leaves_at_the_by_value_width(case, least):
    m = 32
    c = case(m)
    W = engine.pass_width(m)
    assert engine.coalesce_long(least) == 0
    for k in (W + 1, NPATS):
        assert launch_all(c, list(range(k))) == -(-k // W), (least, k)
    assert engine.coalesce_long(0) == least


def test_a_narrower_setting_makes_no_long_pass(case):
    m = 32
    c = case(m)
    assert engine.coalesce_wide(32) == 32  # (the widest, reported as 32)
    assert launch_all(c, list(range(NPATS))) == -(-NPATS // 32)
    assert engine.coalesce_pass(64) == 32
    assert launch_all(c, list(range(NPATS))) == -(-NPATS // 64)
    engine.coalesce_pass(engine.PASS_MAX)
