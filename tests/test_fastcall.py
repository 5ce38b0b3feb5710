"""Plan.launch through smart_amd._fastcall (smart_amd/csrc/fastcall.cpp) against a stub library that records what it was
called with: no GPU.  Every calling form must reach smartgpu_plan_launch with the six values written down here by hand,
through the native binding and — in a child process with SMARTGPU_BINDING=ctypes — through the pure-Python launch;
errors are the library's text as SmartGpuError; integers that do not fit are refused, never folded; no reference is
leaked.  The stub's text is 1000 bytes long, its handles are 0x1000 (text) and 0x2000 (plan)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

STUB_C = r"""
#include <stdint.h>
static uint64_t last[6];
static uint64_t calls;
static int fail;
static const char* error = "";
int smartgpu_plan_launch(void* p, const void* t, uint64_t off, uint64_t n, int slot, int timed)
{
    last[0] = (uint64_t)(uintptr_t)p; last[1] = (uint64_t)(uintptr_t)t; last[2] = off; last[3] = n;
    last[4] = (uint64_t)(int64_t)slot; last[5] = (uint64_t)(int64_t)timed;
    ++calls;
    if (!p || !t) { error = "plan or text is NULL"; return -3; }
    if (fail) { error = "the stub says no"; return -2; }
    return 0;
}
const char* smartgpu_last_error(void) { return error; }
uint64_t smartgpu_text_length(const void* t) { return t ? 1000 : 0; }
void smartgpu_text_free(void* t) { (void)t; }
void smartgpu_plan_free(void* p) { (void)p; }
void stub_last(uint64_t* out) { for (int i = 0; i < 6; ++i) out[i] = last[i]; }
uint64_t stub_calls(void) { return calls; }
void stub_fail(int on) { fail = on; }
"""
TEXT_H, PLAN_H, LEN = 0x1000, 0x2000, 1000
B63 = 1 << 63
# (positional arguments after the text, keyword arguments) -> (off, n, slot, timed) at the library
FORMS = [
    ([], {}, (0, LEN, 0, 0)),
    ([1], {}, (0, LEN, 1, 0)),
    ([], {"slot": 1}, (0, LEN, 1, 0)),
    ([0, True], {}, (0, LEN, 0, 1)),
    ([], {"timed": True}, (0, LEN, 0, 1)),
    ([], {"timed": False}, (0, LEN, 0, 0)),
    ([], {"timed": 1}, (0, LEN, 0, 1)),
    ([], {"timed": 0}, (0, LEN, 0, 0)),
    ([], {"timed": "yes"}, (0, LEN, 0, 1)),
    ([], {"timed": 7, "slot": 1}, (0, LEN, 1, 1)),
    ([], {"off": 10}, (10, LEN - 10, 0, 0)),
    ([], {"off": LEN}, (LEN, 0, 0, 0)),
    ([], {"n": None}, (0, LEN, 0, 0)),
    ([0, False, 10, None], {}, (10, LEN - 10, 0, 0)),
    ([0, False, 10, 5], {}, (10, 5, 0, 0)),
    ([], {"off": 4097, "n": 3}, (4097, 3, 0, 0)),
    ([1], {"n": 7, "off": 3, "timed": 1}, (3, 7, 1, 1)),
    ([], {"n": 0}, (0, 0, 0, 0)),
    ([], {"off": B63, "n": B63 + 5}, (B63, B63 + 5, 0, 0)),
    ([], {"off": 2 ** 64 - 1, "n": 2 ** 64 - 1}, (2 ** 64 - 1, 2 ** 64 - 1, 0, 0)),
    ([], {"slot": 2 ** 31 - 1}, (0, LEN, 2 ** 31 - 1, 0)),
]

# what both processes run: build a Text and a Plan on the stub, make every call of FORMS, return what the stub saw
DRIVER = r"""
import ctypes
def make(engine):
    text = engine.Text(0x1000)
    plan = engine.Plan.__new__(engine.Plan)
    plan._L = engine.lib()
    engine._bind_plan(plan)
    plan._h = 0x2000
    return plan, text
def last(L):
    out = (ctypes.c_uint64 * 6)()
    L.stub_last(out)
    return [int(x) for x in out]
def drive(engine, forms):
    plan, text = make(engine)
    seen = []
    for args, kwargs in forms:
        assert plan.launch(text, *args, **kwargs) is None
        seen.append(last(engine.lib()))
    return seen
"""
exec(DRIVER)


@pytest.fixture(scope="module")
def stub_path(tmp_path_factory):
    d = tmp_path_factory.mktemp("stub")
    src = d / "stub.c"
    src.write_text(STUB_C)
    so = d / "libstub.so"
    subprocess.check_call(["cc", "-O1", "-shared", "-fPIC", "-o", str(so), str(src)])
    return str(so)


@pytest.fixture
def stub(stub_path):
    """The stub as the library new Text / Plan objects go to, for one test."""
    from smart_amd import engine
    before = engine._lib
    L = engine.use_library(stub_path)
    L.stub_calls.restype = ctypes.c_uint64
    L.stub_fail(0)
    try:
        yield L
    finally:
        L.stub_fail(0)
        engine._lib = before


@pytest.fixture
def native(stub):
    from smart_amd import engine
    if engine.binding() != "native":
        pytest.skip("smart_amd._fastcall was not built (no Python.h at build time) or SMARTGPU_BINDING=ctypes is set")
    return engine


def want(form):
    off, n, slot, timed = form[2]
    return [PLAN_H, TEXT_H, off, n, slot, timed]


def test_every_calling_form_reaches_the_library_with_its_six_values(native):
    seen = drive(native, [(a, k) for a, k, _ in FORMS])  # noqa: F821
    assert seen == [want(f) for f in FORMS]
    plan, text = make(native)  # noqa: F821
    plan.launch(text=text, off=1)  # the text by keyword
    assert last(native.lib()) == [PLAN_H, TEXT_H, 1, LEN - 1, 0, 0]  # noqa: F821
    assert text._length() == LEN == len(text)  # (len() asks the current library, which is the stub here)
    assert native.Plan.launch is native._fastcall.PlanBase.launch


def test_the_ctypes_fallback_makes_the_same_calls(stub_path):
    """A child process with SMARTGPU_BINDING=ctypes: binding() says so, and the stub sees the same six values."""
    forms = [(a, k) for a, k, _ in FORMS]
    code = DRIVER + "\nimport json, sys\nfrom smart_amd import engine\n" \
        "print(json.dumps({'binding': engine.binding(), 'seen': drive(engine, json.loads(sys.argv[1]))}))\n"
    env = dict(os.environ, SMARTGPU_BINDING="ctypes", SMARTGPU_LIB=stub_path, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code, json.dumps(forms)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["binding"] == "ctypes"
    assert got["seen"] == [want(f) for f in FORMS]


def test_the_pure_python_launch_in_this_process(stub):
    """Plan._launch_ctypes is today's launch whichever binding is active: the same values again."""
    from smart_amd import engine
    plan, text = make(engine)  # noqa: F821
    for args, kwargs, _ in FORMS:
        plan._launch_ctypes(text, *args, **kwargs)
        assert last(stub) == want((args, kwargs, _))  # noqa: F821


def test_a_failing_launch_raises_the_librarys_text(native, stub):
    plan, text = make(native)  # noqa: F821
    stub.stub_fail(1)
    with pytest.raises(native.SmartGpuError, match=r"^plan_launch: the stub says no$"):
        plan.launch(text)
    stub.stub_fail(0)
    plan.launch(text)


def test_freed_objects_give_the_librarys_error_not_a_crash(native, stub):
    plan, text = make(native)  # noqa: F821
    plan.free()
    assert plan._h is None
    with pytest.raises(native.SmartGpuError, match="plan or text is NULL"):
        plan.launch(text)
    assert last(stub)[:2] == [0, TEXT_H]  # noqa: F821
    plan, text = make(native)  # noqa: F821
    text.free()
    assert text._h is None and text._length() == 0
    with pytest.raises(native.SmartGpuError, match="plan or text is NULL"):
        plan.launch(text)
    assert last(stub)[:2] == [PLAN_H, 0]  # noqa: F821
    with pytest.raises(native.SmartGpuError, match="plan or text is NULL"):
        plan.launch(text, off=0, n=10)
    plan._h = 0x2000  # assignable, with today's meaning
    text._h = TEXT_H
    plan.launch(text)
    assert last(stub) == [PLAN_H, TEXT_H, 0, LEN, 0, 0]  # noqa: F821


def test_arguments_that_do_not_fit_are_refused_not_folded(native, stub):
    plan, text = make(native)  # noqa: F821
    calls = stub.stub_calls()
    for bad in (5, object(), b"abc", None, plan):
        with pytest.raises(TypeError):
            plan.launch(bad)
    for kwargs in ({"off": -1}, {"off": 2 ** 64}, {"n": -1}, {"n": 2 ** 64}, {"off": -2 ** 63}, {"slot": 2 ** 31}, {"slot": -2 ** 31 - 1},
                   {"slot": 2 ** 64}):
        with pytest.raises(OverflowError):
            plan.launch(text, **kwargs)
    with pytest.raises(ValueError):  # n=None behind the text's end has no length to give
        plan.launch(text, off=LEN + 1)
    for kwargs in ({"off": 1.5}, {"n": "3"}, {"slot": 0.0}, {"nope": 1}):
        with pytest.raises(TypeError):
            plan.launch(text, **kwargs)
    with pytest.raises(TypeError):
        plan.launch()
    with pytest.raises(TypeError):
        plan.launch(text, 0, False, 0, None, 1)
    with pytest.raises(TypeError):
        plan.launch(text, 0, slot=1)
    assert stub.stub_calls() == calls  # none of them reached the library
    plan.launch(text, slot=-1)  # (an int: the library decides about its range)
    assert last(stub)[4] == 2 ** 64 - 1  # noqa: F821  (-1, sign-extended by the stub)


def test_handles_are_ints_or_none(native):
    plan, text = make(native)  # noqa: F821
    for obj in (plan, text):
        with pytest.raises(TypeError):
            obj._h = "0x1000"
        with pytest.raises(OverflowError):
            obj._h = -1
        with pytest.raises(OverflowError):
            obj._h = 2 ** 64
    assert plan._h == PLAN_H and text._h == TEXT_H
    unbound = native.Text.__new__(native.Text)
    assert unbound._h is None
    with pytest.raises(RuntimeError):
        unbound._h = TEXT_H  # no length to read yet


def test_no_reference_is_leaked_or_stolen(native, stub):
    plan, text = make(native)  # noqa: F821
    launch = plan.launch
    off, n = 10 ** 15, 10 ** 15 + 1  # (objects of their own, not cached small ints)

    def counts():
        return [sys.getrefcount(x) for x in (plan, text, off, n, None, native.SmartGpuError)]
    before = counts()
    for _ in range(10 ** 5):
        launch(text, 1, True, off, n)
        launch(text, slot=1, off=off, n=n, timed=None)
        launch(text, off=5, n=None)
    mid = counts()
    stub.stub_fail(1)
    for _ in range(10 ** 3):
        try:
            launch(text, off=off, n=n)
        except native.SmartGpuError:
            pass
        try:
            launch(text, off=-1)
        except OverflowError:
            pass
        try:
            launch(None)
        except TypeError:
            pass
    stub.stub_fail(0)
    after = counts()
    # None's count also moves with what the interpreter does around the loop: a leak would be 10^5 (10^3 on the error paths)
    for a, b in ((before, mid), (mid, after)):
        assert a[:4] == b[:4] and abs(a[4] - b[4]) < 100 and abs(a[5] - b[5]) < 100, (before, mid, after)
