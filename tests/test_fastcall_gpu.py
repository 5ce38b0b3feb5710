"""Plan.launch through smart_amd._fastcall on the GPU: the native binding against the pure-Python launch (Plan._launch_ctypes,
what SMARTGPU_BINDING=ctypes runs) and against the oracle's brute force.  Bit-exact.

2 MiB of rand128 and 100 Horspool plans of 32 bytes cut from it, two of them made to repeat their symbols (and planted),
so that they ride in the pass that is gathering.  The same launches through both bindings must give the same counts and
move the queue's counters (launches, passes, riders, sampled passes) alike: 98 launches and 2 riders, 84 entries in a
first pass and 16 in the one the flush sends.  Once over a text created with smartgpu_text_sampling(0) (hor_sample_scan)
and once with the library's default (no sample below 64 MiB: hor_multi_scan).  Also a sub-range, slot 1 of a caller's
result buffer, a timed launch, m = 8, and a launch after free()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from smart_amd import Plan, SmartGpuError, Text, engine  # noqa: E402
from test_coalesce_gram_gpu import need_gpu, streaming  # noqa: E402,F401

SEED = 0x5EEDFA57
N, M, PLANS = 2 << 20, 32, 100
RIDERS = (10, 50)  # which of the 100 repeat their symbols
SUB = (4097, 1 << 20)  # off, n


@pytest.fixture(autouse=True)
def widest_passes():
    if engine.binding() != "native":
        pytest.skip("smart_amd._fastcall was not built (no Python.h at build time) or SMARTGPU_BINDING=ctypes is set")
    width = engine.coalesce_pass(engine.PASS_MAX)
    on = engine.coalesce_sample(True)
    try:
        yield
    finally:
        engine.device_sync(0)
        engine.coalesce_sample(on)
        engine.coalesce_pass(width)


def native(pl):
    return pl.launch


def pure_python(pl):
    return pl._launch_ctypes


class Case:
    def __init__(self, po):
        T = po.gen_text(SEED, 128, 0, N).copy()
        pats = []
        at = 5000
        while len(pats) < PLANS:
            P = T[at:at + M].copy()
            if len(pats) in RIDERS:
                for i in range(6):  # as tests/test_coalesce_ride_gpu.py makes a pattern of 32 bytes repeat
                    P[1 + i * (M // 6)] = P[0]
                assert not streaming(P) and engine.kernel_for("hor", P) == "hor_scan" and len(set(P.tolist())) >= 5
                T[at:at + M] = P
                T[at + 700_000:at + 700_000 + M] = P
                pats.append(P)
            elif streaming(P):
                pats.append(P)
            at += 15_013
        assert at + M < N
        self.T, self.pats = T, pats
        self.want = [po.search("bf", P, T) for P in pats]
        self.want_sub = [po.search("bf", P, T[SUB[0]:SUB[0] + SUB[1]]) for P in pats]
        assert min(self.want) >= 1 and all(self.want[j] >= 2 for j in RIDERS) and sum(self.want_sub) >= 40
        self.texts, self.plans = {}, None

    def text(self, sampling):
        """The text created under smartgpu_text_sampling(sampling); None: the library's setting as it stands."""
        if sampling not in self.texts:
            before = engine.text_sampling(sampling) if sampling is not None else None
            try:
                self.texts[sampling] = Text.upload(self.T)
            finally:
                if before is not None:
                    engine.text_sampling(before)
        if self.plans is None:
            self.plans = [Plan("hor", P) for P in self.pats]
        return self.texts[sampling]

    def run(self, of, text, **kwargs):
        """-> (counts, [launches, passes, riders, sampled passes] the run added)"""
        for pl in self.plans:
            pl.reset()
        engine.device_sync(0)
        before = counters()
        for pl in self.plans:
            of(pl)(text, **kwargs)
        engine.device_sync(0)
        return [pl.result(kwargs.get("slot", 0))[0] for pl in self.plans], (counters() - before).tolist()

    def free(self):
        for pl in self.plans or []:
            pl.free()
        for t in self.texts.values():
            t.free()


def counters():
    launches, passes = engine.coalesce_stats(0)
    return np.array([launches, passes, engine.coalesce_riders(0), engine.coalesce_sampled(0)], dtype=np.int64)


_case = []


@pytest.fixture
def case(oracle):
    if not _case:
        _case.append(Case(oracle))
    return _case[0]


@pytest.mark.parametrize("sampling", (0, None))
def test_both_bindings_count_like_brute_force_and_move_the_counters_alike(case, sampling):
    setting = engine.text_sampling(-1)  # (reads the setting ...
    engine.text_sampling(setting)       # ... and puts it back)
    text = case.text(sampling)
    assert engine.text_sampling(setting) == setting  # the case restored it
    sampled = engine.text_has_sample(text)
    assert sampled == (sampling == 0)
    got_n, moved_n = case.run(native, text)
    got_p, moved_p = case.run(pure_python, text)
    assert got_n == case.want and got_p == case.want
    assert moved_n == moved_p == [PLANS - len(RIDERS), 2, len(RIDERS), 2 if sampled else 0]


@pytest.mark.parametrize("sampling", (0, None))
def test_a_sub_range(case, sampling):
    text = case.text(sampling)
    got_n, moved_n = case.run(native, text, off=SUB[0], n=SUB[1])
    got_p, moved_p = case.run(pure_python, text, off=SUB[0], n=SUB[1])
    assert got_n == case.want_sub and got_p == case.want_sub and moved_n == moved_p
    # n=None: to the end of the text, from the length the text base read when the handle was set
    got_n, _ = case.run(native, text, off=SUB[0])
    got_p, _ = case.run(pure_python, text, off=SUB[0], n=N - SUB[0])
    assert got_n == got_p and text._length() == N == len(text)


def test_slot_1_of_a_callers_result_buffer(case):
    text = case.text(0)
    holder = Plan("hor", case.pats[0])  # its zeroed result slots serve as the caller's device buffer
    mine = case.plans[:5]
    try:
        for j, pl in enumerate(mine):
            pl.set_result_buffer(holder.result_device_ptr + 8 * (40 + 2 * j), 2)
        for pl in mine:
            pl.launch(text, slot=1)
            pl._launch_ctypes(text, slot=1)
            pl.launch(text, 0)
        engine.device_sync(0)
        assert [holder.result(41 + 2 * j)[0] for j in range(5)] == [2 * w for w in case.want[:5]]
        assert [holder.result(40 + 2 * j)[0] for j in range(5)] == case.want[:5]
        with pytest.raises(SmartGpuError, match="slot 2 out of range"):
            mine[0].launch(text, slot=2)
    finally:
        for pl in mine:
            pl.set_result_buffer(None, 0)
        holder.free()


def test_a_timed_launch(case):
    text = case.text(0)
    pl = case.plans[3]
    pl.reset()
    pl.launch(text, timed=True)
    count, ms = pl.result(0)
    assert count == case.want[3] and ms > 0
    pl.launch(text, 0, 1)  # timed, by position
    count, ms = pl.result(0)
    assert count == 2 * case.want[3] and ms > 0


def test_patterns_of_8_bytes_the_unsampled_path(case, oracle):
    text = case.text(0)
    pats = []
    at = 9000
    while len(pats) < 6:
        P = case.T[at:at + 8].copy()
        if streaming(P):
            pats.append(P)
        at += 30_011
    plans = [Plan("hor", P) for P in pats]
    try:
        counts = {}
        for name, of in (("native", native), ("python", pure_python)):
            for pl in plans:
                pl.reset()
            engine.device_sync(0)
            before = counters()
            for pl in plans:
                of(pl)(text)
            engine.device_sync(0)
            counts[name] = [pl.result(0)[0] for pl in plans]
            assert (counters() - before).tolist() == [6, 1, 0, 0]  # one shared pass, not over the sample
        assert counts["native"] == counts["python"] == [oracle.search("bf", P, case.T) for P in pats]
    finally:
        for pl in plans:
            pl.free()


def test_a_launch_after_free_raises(case):
    text = case.text(0)
    pl = Plan("hor", case.pats[1])
    pl.launch(text)
    pl.free()
    assert pl._h is None
    with pytest.raises(SmartGpuError, match="plan_launch: plan or text is NULL"):
        pl.launch(text)
    gone = Text.upload(case.T[:4096])
    gone.free()
    with pytest.raises(SmartGpuError, match="plan_launch: plan or text is NULL"):
        case.plans[0].launch(gone)
    with pytest.raises(TypeError):
        case.plans[0].launch(case.T)


def test_free_the_shared_case():
    for c in _case:
        c.free()
    _case.clear()
