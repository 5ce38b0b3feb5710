"""An untimed launch that cannot share a pass — another algorithm, a Horspool pattern whose symbols repeat — goes to the
stream at once and sends nothing that is pending (smartgpu_plan_launch, api.cpp): the key goes on gathering across it, so
eight streaming launches make ONE pass whatever is launched between them.  Every count against the oracle's brute force.
Bit-exact.  Texts, patterns and plans are those of tests/test_coalesce_gpu.py (3 * 16384 + 777 bytes, and 5000 bytes);
m = 17 (the whole window in LDS), 32 (the headline: one of bench.py's 250 patterns repeats its symbols) and 100."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from smart_amd import Plan, engine  # noqa: E402
from test_coalesce_gpu import N_BIG, N_SMALL, Case, groups_of_eight, need_gpu, streaming  # noqa: E402,F401

MS = (17, 32, 100)
_cases = {}


class Mixed:
    """A case of test_coalesce_gpu.py plus three plans that never share a pass, with their brute-force counts."""

    def __init__(self, po, n, m):
        self.c = c = Case(po, n, m)
        R = c.T[1000:1000 + m].copy()  # a Horspool pattern whose symbols repeat: hor_scan, not its streaming form
        copies = {17: 3, 32: 6, 100: 16}[m]
        for i in range(copies):
            R[1 + i * (m // copies)] = R[0]
        assert not streaming(R) and engine.kernel_for("hor", R) == "hor_scan"
        self.pats = [R, c.pats[0], c.pats[1]]
        self.others = [Plan("hor", R), Plan("kmp", c.pats[0]), Plan("bm", c.pats[1])]
        self.want = [po.search("bf", P, c.T) for P in self.pats]

    def reset(self):
        for pl in self.c.plans + self.others:
            pl.reset()
        engine.device_sync(0)


@pytest.fixture
def mixed(oracle):
    def get(n, m):
        if (n, m) not in _cases:
            _cases[(n, m)] = Mixed(oracle, n, m)
        return _cases[(n, m)]
    return get


@pytest.mark.parametrize("n", (N_BIG, N_SMALL))
@pytest.mark.parametrize("m", MS)
def test_a_launch_that_cannot_share_does_not_split_a_pass(mixed, m, n):
    x = mixed(n, m)
    c = x.c
    x.reset()
    l0, p0 = engine.coalesce_stats(0)
    for j, pl in enumerate(c.plans[:8]):
        pl.launch(c.text)
        if j in (2, 4, 6):
            x.others[j // 2 - 1].launch(c.text)
    engine.device_sync(0)
    l1, p1 = engine.coalesce_stats(0)
    assert [pl.result(0)[0] for pl in c.plans[:8]] == c.want[:8], (m, n)
    assert [pl.result(0)[0] for pl in x.others] == x.want, (m, n)
    assert (l1 - l0, p1 - p0) == (8, 1)  # the three are no launches that could share, and they sent nothing


@pytest.mark.parametrize("m", MS)
def test_seventeen_launches_with_others_between_make_three_passes(mixed, m):
    x = mixed(N_BIG, m)
    c = x.c
    x.reset()
    l0, p0 = engine.coalesce_stats(0)
    for j, pl in enumerate(c.plans):
        pl.launch(c.text)
        x.others[j % 3].launch(c.text)
    l1, p1 = engine.coalesce_stats(0)  # nothing waited yet: two full passes were sent, one launch is pending
    assert (l1 - l0, p1 - p0) == (17, 2)
    assert [pl.result(0)[0] for pl in x.others] == [w * len(range(k, 17, 3)) for k, w in enumerate(x.want)], m
    assert [pl.result(0)[0] for pl in c.plans] == c.want, m
    assert engine.coalesce_stats(0)[1] - p0 == 3  # 8 + 8 + 1


def test_a_timed_launch_still_sends_what_is_pending(mixed):
    x = mixed(N_BIG, 32)
    c = x.c
    x.reset()
    l0, p0 = engine.coalesce_stats(0)
    c.plans[0].launch(c.text)
    c.plans[1].launch(c.text)
    x.others[1].launch(c.text, timed=True)  # its events bracket its own kernel, behind the pass of two
    assert engine.coalesce_stats(0)[1] - p0 == 1
    c.plans[2].launch(c.text)
    c.plans[3].launch(c.text)
    count, ms = x.others[1].result(0)
    assert count == x.want[1] and ms > 0
    assert [pl.result(0)[0] for pl in c.plans[:4]] == c.want[:4]
    l1, p1 = engine.coalesce_stats(0)
    assert (l1 - l0, p1 - p0) == (4, 2)


def test_one_slot_for_a_queued_and_an_unqueued_launch(mixed):
    """Counts are added: a streaming plan (held back) and the repeating pattern's plan (sent at once) share one slot."""
    x = mixed(N_BIG, 32)
    c = x.c
    holder = Plan("hor", c.pats[0])  # its zeroed result slots serve as the caller's device buffer
    slot = holder.result_device_ptr + 8 * 30
    c.plans[0].set_result_buffer(slot, 1)
    x.others[0].set_result_buffer(slot, 1)
    try:
        c.plans[0].launch(c.text)
        x.others[0].launch(c.text)
        c.plans[0].launch(c.text)
        engine.device_sync(0)
        assert holder.result(30)[0] == 2 * c.want[0] + x.want[0]
    finally:
        c.plans[0].set_result_buffer(None, 0)
        x.others[0].set_result_buffer(None, 0)
        holder.free()
