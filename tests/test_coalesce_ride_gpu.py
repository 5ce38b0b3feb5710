"""Riders: a Horspool pattern whose own symbols repeat, over a text whose symbols do not (its measured rate at most 1/48),
joins the key that is gathering for its text, range and length and leaves with that key's pass (api.cpp queue_launch).
It opens no key, counts neither in coalesce_stats' launches nor toward the coalesce setting, and is reported by
coalesce_riders.  Every count against the oracle's brute force.  Bit-exact.

NOT observed here: the name of any kernel.  That the kernels sent are hor_multi_scan only is INFERRED from the library's
own counters (below), which is bookkeeping of the code under test; what is independent of it are the counts — a rider
that was queued and also sent alone, or dropped, shows in its doubled or tripled count — and the kernel traces of
profiles/coalesce/RESULTS.md ("Riders"), which show no hor_scan where every repeating launch had a key.

Texts of 3 * 16384 + 777 and of 5000 bytes, as tests/test_coalesce_gpu.py has them (its cases' patterns and plans are shared);
m = 8 (the shortest rider), 17 (the whole window in LDS), 32 (the headline), 100 (completion in memory).

Which kernels ran is read from the counters, which account for every launch: a launch is a streaming one (launches),
a rider (riders) or went alone.  Where riders rises by the number of repeating launches none of them went alone, and
where passes rises by the number of keys sent, each with two entries or more, every kernel was a hor_multi_scan.

The pattern that occurs often.  A pattern (x y)^(m/2) has two symbols, so its plan carries Horspool's q-gram table
(plan.cpp build_blob: q = 8 from 16 bytes on) and its route is {hor, 8}, not the {hor, 0} a pass takes: by the rider's
own rules it never rides.  It is launched here all the same, twice, between the launches of a pass, and counted: it
goes alone.  The frequent RIDER is the nearest pattern that can ride: period nine over nine symbols (fewer than nine
symbols in 32 bytes or more leave hor_scan's route), with a planted run of that period of 3000 bytes (400 in the small
text) across a tile boundary: about 330 overlapping occurrences, seven to a lane's 64 window ends and in every lane of
the waves over the run — many adds to one LDS counter, a parked candidate in every lane of a wave and completion in
memory for the lane's further ones."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from smart_amd import Plan, Text, engine  # noqa: E402
from test_coalesce_gpu import N_BIG, N_SMALL, TILE, case, cut, groups_of_eight, need_gpu, streaming  # noqa: E402,F401

MS = (8, 17, 32, 100)
SEED = 0x5EED21DE


def rate_of(T):
    """sum c (c - 1) / (N (N - 1)) over the byte histogram of T, as text_rate.hpp has it."""
    c = np.bincount(T, minlength=256).astype(np.float64)
    return float((c * (c - 1)).sum() / (len(T) * (len(T) - 1.0)))


def can_ride(P):
    """A Horspool pattern whose symbols repeat by build_blob's rule and whose route is still {hor, 0}: hor_scan's
    verifying form with the byte table (five symbols or more: no q-gram table)."""
    return not streaming(P) and engine.kernel_for("hor", P) == "hor_scan" and len(set(P.tolist())) >= 5


def repeating(T, m, at=1000):
    """A pattern cut from T whose symbols repeat, built as tests/test_coalesce_order_gpu.py builds its R."""
    R = T[at:at + m].copy()
    copies = {8: 1, 17: 3, 32: 6, 100: 16}[m]
    for i in range(copies):
        R[1 + i * (m // copies)] = R[0]
    return R


def streams(text):
    rate = text.repeat_rate()
    return rate is not None and rate * 48 <= 1


def counters():
    launches, passes = engine.coalesce_stats(0)
    return np.array([launches, passes, engine.coalesce_riders(0)], dtype=np.int64)


class Ride:
    """A case of test_coalesce_gpu.py (a rand128 text with planted copies, 17 streaming patterns and their plans) with a
    repeating pattern planted three times in a copy of its text."""

    def __init__(self, po, c):
        self.m = c.m
        self.R = repeating(c.T, c.m)
        assert can_ride(self.R), c.m
        # the case's text with three copies of R between its planted patterns; its plans, and their counts on THIS text
        T = c.T.copy()
        taken = [(e - c.m + 1, e) for e in c.ends]
        for at in ((2000, 7000, 11000) if c.n == N_BIG else (300, 1700, 4000)):
            assert all(at + c.m <= a or at > b for a, b in taken), (at, taken)
            T[at:at + c.m] = self.R
        self.T, self.plans = T, c.plans
        self.text = Text.upload(T)
        self.rplan = Plan("hor", self.R)
        self.want = [po.search("bf", P, T) for P in c.pats]
        self.want_r = po.search("bf", self.R, T)
        assert self.want_r >= 3 and self.want[0] >= len(c.ends) and sum(w >= 1 for w in self.want) >= 12
        rate = self.text.repeat_rate()
        assert streams(self.text) and abs(rate - rate_of(T)) < 1e-12, (rate, rate_of(T))  # counted whole: exact

    def reset(self):
        for pl in self.plans + [self.rplan]:
            pl.reset()
        engine.device_sync(0)


_rides = {}


@pytest.fixture
def ride(case, oracle):
    def get(n, m):
        if (n, m) not in _rides:
            _rides[(n, m)] = Ride(oracle, case(n, m))
        return _rides[(n, m)]
    return get


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
@pytest.mark.parametrize("m", MS)
def test_riders_in_a_pass(ride, m, n):
    x = ride(n, m)
    c = x
    x.reset()
    before = counters()
    for j, pl in enumerate(c.plans[:8]):
        pl.launch(c.text)
        if j in (0, 2, 5):
            x.rplan.launch(c.text)
    sent = counters() - before  # the eighth streaming launch sent the key, eleven entries in it: nothing waited yet
    assert sent.tolist() == [8, 1, 3], (m, n)
    engine.device_sync(0)
    assert (counters() - before).tolist() == [8, 1, 3]  # as if the riders were not there; one kernel, a hor_multi_scan
    assert [pl.result(0)[0] for pl in c.plans[:8]] == c.want[:8], (m, n)
    assert x.rplan.result(0)[0] == 3 * x.want_r, (m, n)


def test_riders_and_the_width_of_a_key(ride):
    x = ride(N_BIG, 32)
    c = x
    x.reset()
    prev = engine.coalesce_pass(96)
    try:
        assert engine.pass_width(32) == 84
        before = counters()
        times = [0] * len(c.plans)
        for j in range(80):
            c.plans[j % len(c.plans)].launch(c.text)
            times[j % len(c.plans)] += 1
            if j == 77:  # 78 streaming launches and five riders wait: neither the setting nor the room is reached
                assert (counters() - before).tolist() == [78, 0, 5]
            if j in (5, 20, 35, 50, 65, 77):
                x.rplan.launch(c.text)
        # the sixth rider was the 84th entry and sent the key; two streaming launches came after it
        assert (counters() - before).tolist() == [80, 1, 6]
        engine.device_sync(0)
        assert (counters() - before).tolist() == [80, 2, 6]  # the rest left at the sync, a pass of two
        assert [pl.result(0)[0] for pl in c.plans] == [w * t for w, t in zip(c.want, times)]
        assert x.rplan.result(0)[0] == 6 * x.want_r
    finally:
        engine.device_sync(0)
        engine.coalesce_pass(prev)


@pytest.mark.parametrize("m", MS)
def test_a_rider_with_no_key_goes_alone(ride, m):
    x = ride(N_BIG, m)
    c = x
    x.reset()
    before = counters()
    x.rplan.launch(c.text)  # the first launch after a sync: nothing is gathering
    assert (counters() - before).tolist() == [0, 0, 0]
    for pl in c.plans[:8]:
        pl.launch(c.text)
    assert (counters() - before).tolist() == [8, 1, 0]
    x.rplan.launch(c.text)  # right after a key was sent
    assert (counters() - before).tolist() == [8, 1, 0]
    c.plans[8].launch(c.text)
    x.rplan.launch(c.text)  # this one has a key
    engine.device_sync(0)
    assert (counters() - before).tolist() == [9, 2, 1]
    assert x.rplan.result(0)[0] == 3 * x.want_r and [pl.result(0)[0] for pl in c.plans[:9]] == c.want[:9], m


def test_a_timed_rider_is_not_a_rider(ride):
    x = ride(N_BIG, 32)
    c = x
    x.reset()
    before = counters()
    c.plans[0].launch(c.text)
    c.plans[1].launch(c.text)
    x.rplan.launch(c.text, timed=True)  # sends the two, then runs alone between its events
    assert (counters() - before).tolist() == [2, 1, 0]
    count, ms = x.rplan.result(0)
    assert count == x.want_r and ms > 0
    assert [pl.result(0)[0] for pl in c.plans[:2]] == c.want[:2]


class Frequent:
    """A rand128 text with two planted runs, x y x y ... and a run of period nine, each 3000 bytes (400 in the small text)
    across a tile boundary (the small text: across 64-byte boundaries), three streaming patterns cut in front of them,
    and the two periodic patterns of m bytes."""

    def __init__(self, po, n, m):
        T = po.gen_text(SEED + m, 128, 0, n).copy()
        run = 3000 if n == N_BIG else 400
        xy_at, nine_at = (TILE - 1500 - 1, 2 * TILE - 1500 - 3) if n == N_BIG else (1001, 3003)
        unit = np.arange(97, 106, dtype=np.uint8)
        T[xy_at:xy_at + run] = np.resize(np.array([65, 66], dtype=np.uint8), run)
        T[nine_at:nine_at + run] = np.resize(unit, run)
        self.T, self.run = T, run
        self.XY = np.resize(np.array([65, 66], dtype=np.uint8), m)
        self.F = np.resize(unit, m)
        assert can_ride(self.F) and not streaming(self.XY) and len(set(self.XY.tolist())) == 2
        self.pats = [cut(T, k, m) for k in (100, 400, 700)]
        self.want = [po.search("bf", P, T) for P in self.pats]
        self.want_xy, self.want_f = po.search("bf", self.XY, T), po.search("bf", self.F, T)
        assert self.want_xy >= (run - m) // 2 + 1 and self.want_f >= (run - m) // 9 + 1
        self.text = Text.upload(T)
        assert streams(self.text) and self.text.repeat_rate() < 0.013, self.text.repeat_rate()
        self.plans = [Plan("hor", P) for P in self.pats]
        self.xy, self.f = Plan("hor", self.XY), Plan("hor", self.F)


_frequent = {}


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
@pytest.mark.parametrize("m", (32, 100))
def test_a_rider_that_occurs_often(oracle, m, n):
    if (n, m) not in _frequent:
        _frequent[(n, m)] = Frequent(oracle, n, m)
    x = _frequent[(n, m)]
    for pl in x.plans + [x.xy, x.f]:
        pl.reset()
    engine.device_sync(0)
    before = counters()
    x.plans[0].launch(x.text)
    x.f.launch(x.text)
    x.plans[1].launch(x.text)
    x.xy.launch(x.text)  # two symbols: Horspool's q-gram table, route {hor, 8}: alone
    x.f.launch(x.text)   # the same pattern twice in one pass: twice on its chain
    x.xy.launch(x.text)
    x.plans[2].launch(x.text)
    engine.device_sync(0)
    assert (counters() - before).tolist() == [3, 1, 2], (m, n)
    assert x.f.result(0)[0] == 2 * x.want_f, (m, n, x.want_f)
    assert x.xy.result(0)[0] == 2 * x.want_xy, (m, n, x.want_xy)
    assert [pl.result(0)[0] for pl in x.plans] == x.want, (m, n)


class Gated:
    """A text whose rate lies ABOVE 1/48 — rand32, or rand128 with a run of one symbol over 14 % of it — with two
    streaming patterns planted once each (they need not be cut from the text: m distinct byte values) and a repeating one."""

    def __init__(self, po, kind, n, m):
        if kind == "rand32":
            T = po.gen_text(SEED + 32 + m, 32, 0, n).copy()
        else:
            T = po.gen_text(SEED + 128 + m, 128, 0, n).copy()
            run = int(0.14 * n)
            T[n - 300 - run:n - 300] = 77
        self.pats = [((np.arange(m) + 40 + 110 * j) % 256).astype(np.uint8) for j in range(2)]
        for j, P in enumerate(self.pats):
            assert streaming(P)
            T[200 + 150 * j:200 + 150 * j + m] = P
        self.T = T
        self.R = repeating(T, m, at=1000)
        assert can_ride(self.R), (kind, m)  # only the text keeps it out
        T[2500:2500 + m] = self.R
        assert rate_of(T) * 48 > 1.1, (kind, rate_of(T))
        self.text = Text.upload(T)
        assert self.text.repeat_rate() is not None and not streams(self.text), self.text.repeat_rate()
        self.plans = [Plan("hor", P) for P in self.pats]
        self.rplan = Plan("hor", self.R)
        self.want = [po.search("bf", P, T) for P in self.pats]
        self.want_r = po.search("bf", self.R, T)
        assert min(self.want) >= 1 and self.want_r >= 1


_gated = {}


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("kind", ("rand32", "run"))
def test_the_gate(oracle, kind, m, n):
    if (kind, n, m) not in _gated:
        _gated[(kind, n, m)] = Gated(oracle, kind, n, m)
    x = _gated[(kind, n, m)]
    for pl in x.plans + [x.rplan]:
        pl.reset()
    engine.device_sync(0)
    before = counters()
    x.plans[0].launch(x.text)
    x.rplan.launch(x.text)  # a key is gathering, but this text's symbols repeat: alone
    x.plans[1].launch(x.text)
    engine.device_sync(0)
    assert (counters() - before).tolist() == [2, 1, 0], (kind, m, n)
    assert x.rplan.result(0)[0] == x.want_r and [pl.result(0)[0] for pl in x.plans] == x.want, (kind, m, n)


def test_upload_and_generate_report_one_rate(oracle):
    for sigma, n in ((128, N_BIG), (48, N_SMALL), (32, N_BIG)):
        T = oracle.gen_text(SEED + sigma, sigma, 0, n)
        up, gen = Text.upload(T), Text.generate(SEED + sigma, sigma, n)
        assert up.repeat_rate() == gen.repeat_rate() and abs(up.repeat_rate() - rate_of(T)) < 1e-12, (sigma, n)
        assert abs(up.repeat_rate() - 1.0 / sigma) < 0.1 / sigma
        up.free()
        gen.free()
    # the shortest texts: no rate below two bytes
    for data, want in ((b"", None), (b"a", None), (b"ab", 0.0), (b"aa", 1.0), (b"abcabcabcabcabcabc", rate_of(np.frombuffer(b"abcabcabcabcabcabc", np.uint8)))):
        t = Text.upload(np.frombuffer(data, dtype=np.uint8))
        got = t.repeat_rate()
        assert (got is None) if want is None else abs(got - want) < 1e-12, (data, got)
        t.free()


def test_a_long_text_is_sampled():
    """17 MiB: 2^20 chunks at an even stride, not the whole text.  Its two halves differ (rand128, then rand32), so a
    sample that left a part of the text out would miss the whole text's rate, which numpy computes, by far more than 2 %."""
    n = 17 << 20
    rng = np.random.default_rng(21)
    T = np.concatenate([rng.integers(0, 128, n // 2, dtype=np.uint8), rng.integers(0, 32, n - n // 2, dtype=np.uint8)])
    whole = rate_of(T)
    assert abs(rate_of(T[:n // 2]) - whole) > 0.3 * whole
    t = Text.upload(T)
    got = t.repeat_rate()
    t.free()
    assert got is not None and abs(got - whole) <= 0.02 * whole, (got, whole)
