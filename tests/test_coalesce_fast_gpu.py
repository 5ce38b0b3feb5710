"""Rule (c) of the long passes (api.cpp, above QueuedScan): a key whose launches arrive faster than the GPU could use an
early pass does not send one at pass_width(m); it gathers on to long_width(m), or to the flush.  The launch that fills
the key compares what the GPU would idle meanwhile, at the rate the launches came, with what a pass over the range takes
(the bytes it reads at 4.4 TB/s; never below 10 us).

256 MiB of rand128 created WITHOUT a sample, 100 Horspool plans of 32 bytes read from it (pass_width 84, long_width 152):
* through the native binding 84 launches take a few microseconds, 68 more as many again, against an estimate of 61 us
  for the pass (268 MB / 4.4 TB/s): ONE pass of 100, in the long layout — a margin of ten and more;
* over the first 65 MiB the estimate is 15 us; through the pure-Python launch (0.7 us a launch, 68 of them 48 us) the
  key is sent at 84 as ever: TWO passes.  A slower host only widens that margin;
* over the first 32 MiB, with long passes over any range (smartgpu_coalesce_long(0)), the estimate lies below 10 us and
  decides nothing: two passes through either binding;
* with long passes off (smartgpu_coalesce_long(-1)) two passes whatever the rate.
Every count equals a solo search of the same pattern (smartgpu_search64: hor_scan, no queue) — all 100 over 65 MiB, ten
of them over the whole text — and the two-pass counts equal the one-pass counts.  No sleep, no clock in the test: the
rates differ by the bindings' own cost."""
import pytest

pytestmark = pytest.mark.gpu

from smart_amd import Plan, Text, engine  # noqa: E402
from test_coalesce_gram_gpu import need_gpu, streaming  # noqa: E402,F401

SEED = 0x5EEDFA58
N, M, PLANS = 256 << 20, 32, 100


@pytest.fixture(autouse=True)
def default_rule():
    if engine.binding() != "native":
        pytest.skip("smart_amd._fastcall was not built (no Python.h at build time) or SMARTGPU_BINDING=ctypes is set")
    width = engine.coalesce_pass(engine.PASS_MAX)
    least = engine.coalesce_long(engine.LONG_DEFAULT)
    try:
        yield
    finally:
        engine.device_sync(0)
        engine.coalesce_long(least)
        engine.coalesce_pass(width)


_case = {}


@pytest.fixture
def case():
    if not _case:
        before = engine.text_sampling(-1)
        try:
            text = Text.generate(SEED, 128, N)
        finally:
            engine.text_sampling(before)
        assert not engine.text_has_sample(text) and engine.pass_width(M) == 84 and engine.long_width(M) == 152
        pats, at = [], 7000
        while len(pats) < PLANS:
            P = text.read(at, M)
            if streaming(P):
                pats.append(P)
            at += 600_011  # (the first 100 lie within 64 MiB)
        assert at < 64 << 20
        _case.update(text=text, plans=[Plan("hor", P) for P in pats], pats=pats)
    return _case


def run(case, of, n):
    """-> (counts, passes sent) of one launch of every plan over text[0..n)"""
    for pl in case["plans"]:
        pl.reset()
    engine.device_sync(0)  # (a flush: the key that comes is the first since)
    before = engine.coalesce_stats(0)
    calls, text = [of(pl) for pl in case["plans"]], case["text"]
    for call in calls:
        call(text, 0, False, 0, n)
    engine.device_sync(0)
    after = engine.coalesce_stats(0)
    assert after[0] - before[0] == PLANS
    return [pl.result(0)[0] for pl in case["plans"]], after[1] - before[1]


def native(pl):
    return pl.launch


def pure_python(pl):
    return pl._launch_ctypes


def test_fast_launches_leave_in_one_pass(case):
    got, passes = run(case, native, N)
    assert passes == 1 and min(got) >= 1
    for j in range(0, PLANS, 10):
        assert got[j] == engine.search("hor", case["pats"][j], case["text"])[0], j
    engine.coalesce_long(-1)  # no long passes: 84 + 16
    two, passes = run(case, native, N)
    assert passes == 2 and two == got


def test_slow_launches_send_the_first_pass_at_its_width(case):
    n = 65 << 20
    want = [engine.search("hor", P, case["text"], 0, n)[0] for P in case["pats"]]
    assert min(want) >= 1
    got, passes = run(case, pure_python, n)
    assert got == want and passes == 2
    got, passes = run(case, native, n)  # (15 us against three or four: one pass, mostly; the margin is too thin to assert)
    assert got == want and passes in (1, 2)


def test_a_short_range_is_sent_as_ever(case):
    n = 32 << 20
    engine.coalesce_long(0)
    got, passes = run(case, native, n)
    slow, slow_passes = run(case, pure_python, n)
    assert passes == slow_passes == 2 and got == slow
    assert got[:20] == [engine.search("hor", P, case["text"], 0, n)[0] for P in case["pats"][:20]]


def test_free_the_shared_case():
    for pl in _case.get("plans", []):
        pl.free()
    if _case:
        _case["text"].free()
    _case.clear()
