"""The contract every find call shares (find_run in match_calls.cpp), stated once through the C ABI: pfind64, pfind_sets64,
pfind_mis64 and pfind_sets_mis64 on a two-plane and on a three-plane text, pfind_edit64, pfind_sets_edit64, pfind_editl64,
pfind_sets_editl64, and on the same symbols as a byte text find_edit64, find_edit_classes64, find_editl64,
find_editl_classes64, find_mis64 and find_mis_classes64.

  cap = count      SMARTGPU_OK, the full ascending list (and its distances)
  cap = count - 1  SMARTGPU_ERR_NOMEM, *count = count, the message names both numbers
  cap = 0, NULL    SMARTGPU_ERR_NOMEM, *count = count
  always           the guard words behind the buffers are intact, and the matching count call returns the same number

The text has 3 * 8192 + 300 symbols over four values (six for three planes) and the range starts at 129: the smallest shape in
which a find's entries come from three spans (planes.hpp: kFindSpan start positions from the 128 boundary below the range)
that can reach the cursor out of order, the first of them beginning off a 128 boundary.  Every span holds a copy of the
pattern, one span a second copy with a substitution.  m = 33 is the first length that stages a pattern, m = 70 is beyond the
short edit kernels; k = 1.  The expected lists are definitions in numpy: positions_by_definition (test_packed_find_gpu.py),
by_definition (test_packed_wide_gpu.py; for the byte text's mismatch calls the one of test_text_mis_gpu.py) and the
dynamic-programming row edit_row (test_packed_edit.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import PackedText, Text, byte_classes  # noqa: E402

from test_packed_edit import byte_accepts, edit_row, set_accepts  # noqa: E402
from test_packed_find_gpu import positions_by_definition  # noqa: E402
from test_packed_wide_gpu import by_definition, sets_of  # noqa: E402
from test_text_edit_gpu import class_accepts  # noqa: E402
import test_text_mis_gpu as text_mis  # noqa: E402

OK, ERR_NOMEM = 0, -5
SPAN, OFF, K = 8192, 129, 1
N = 3 * SPAN + 300
VALUES = {False: (65, 67, 71, 84), True: (45, 65, 67, 71, 78, 84)}  # wide: three planes
GUARD64, GUARD8, GUARDS = 0xDEADBEEFDEADBEEF, 0xA5, 4

# name of the find call: (name of the count call, three-plane text as well, pattern kind, m, arguments between m and the
# text, reports distances, what its entries are)
CALLS = {
    "pfind64": ("psearch64", True, "bytes", 33, (), False, "starts"),
    "pfind_sets64": ("psearch_sets64", True, "sets", 33, (), False, "starts"),
    "pfind_mis64": ("psearch_mis64", True, "bytes", 33, (K,), True, "starts"),
    "pfind_sets_mis64": ("psearch_sets_mis64", True, "sets", 33, (K,), True, "starts"),
    "pfind_edit64": ("psearch_edit64", False, "bytes", 33, (K,), True, "ends"),
    "pfind_sets_edit64": ("psearch_sets_edit64", False, "sets", 33, (K,), True, "ends"),
    "pfind_editl64": ("psearch_editl64", False, "bytes", 70, (K, 0), True, "ends"),
    "pfind_sets_editl64": ("psearch_sets_editl64", False, "sets", 70, (K, 0), True, "ends"),
    "find_edit64": ("search_edit64", False, "bytes", 33, (K,), True, "ends"),
    "find_edit_classes64": ("search_edit_classes64", False, "classes", 33, (K,), True, "ends"),
    "find_editl64": ("search_editl64", False, "bytes", 70, (K, 0), True, "ends"),
    "find_editl_classes64": ("search_editl_classes64", False, "classes", 70, (K, 0), True, "ends"),
    "find_mis64": ("search_mis64", False, "bytes", 33, (K,), True, "starts"),
    "find_mis_classes64": ("search_mis_classes64", False, "classes", 33, (K,), True, "starts"),
}
CASES = [(name, wide) for name, c in CALLS.items() for wide in ((False, True) if c[1] else (False,))]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def make_text(wide, m):
    """(T, P): a random text over the values with P at a place of each of the range's three spans and, in the second span, once
    more with its middle symbol substituted."""
    vals = VALUES[wide]
    rng = np.random.default_rng(9000 + 2 * m + wide)
    T = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), N)]
    P = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), m)]
    base = OFF // 128 * 128
    for span in range(3):
        at = base + span * SPAN + 1000 + 37 * span
        T[at:at + m] = P
    W = P.copy()
    W[m // 2] = next(v for v in vals if v != P[m // 2])
    at = base + SPAN + 5000
    T[at:at + m] = W
    T.setflags(write=False)
    return T, P


def widened(P, vals, rng):
    """P as sets: the singleton of each symbol's code, every fifth position with one more member."""
    sets = sets_of(P, vals)
    for j in range(0, len(P), 5):
        sets[j] |= 1 << int(rng.integers(0, len(vals)))
    return sets


@pytest.fixture(scope="module")
def world():
    """Per (wide, m): the text, the pattern in its three kinds, the device texts.  Built on first use, freed at the end."""
    made, handles = {}, []

    def get(wide, m):
        if (wide, m) not in made:
            T, P = make_text(wide, m)
            pt = PackedText.upload(T, wide=wide)
            bt = None if wide else Text.upload(T)
            handles.extend(h for h in (pt, bt) if h is not None)
            sets = widened(P, VALUES[wide], np.random.default_rng(m))
            made[wide, m] = dict(T=T, bytes=P, sets=sets, classes=byte_classes(P, ignore_case=True), packed=pt, text=bt)
        return made[wide, m]
    yield get
    for h in handles:
        h.free()


def expected(name, wide, w):
    """(entries as uint64, distances as uint8) by definition over the range [OFF, N)."""
    _, _, kind, m, extra, dist, what = CALLS[name]
    T, vals, k, ln = w["T"], VALUES[wide], (extra[0] if extra else 0), N - OFF
    if name.startswith("find_mis"):  # a byte text: the window's bytes against the pattern's bytes or classes
        accepts = text_mis.byte_accepts(w["bytes"]) if kind == "bytes" else text_mis.class_accepts(w["classes"])
        return text_mis.by_definition(m, accepts, T, k, OFF, ln)
    if what == "starts":
        if kind == "bytes" and not extra:
            pos = positions_by_definition(w["bytes"], T, OFF, ln)
            return pos, np.zeros(len(pos), dtype=np.uint8)
        return by_definition(w["sets"] if kind == "sets" else sets_of(w["bytes"], vals), T, vals, k, OFF, ln)
    accepts = {"bytes": lambda: byte_accepts(w["bytes"]), "sets": lambda: set_accepts(w["sets"], sorted(vals)),
               "classes": lambda: class_accepts(w["classes"])}[kind]()
    D = edit_row(m, accepts, T, OFF, ln)
    at = np.flatnonzero(D <= k)
    return (at + OFF).astype(np.uint64), D[at].astype(np.uint8)


def find_c(name, w, cap):
    """The find call itself: (rc, count, entries buffer, distances buffer or None, message); cap + GUARDS elements each,
    pre-filled with guard values, NULL at cap = 0."""
    _, _, kind, m, extra, dist, _ = CALLS[name]
    pat = np.ascontiguousarray(w[kind], dtype=np.uint8)
    handle = (w["text"] if name.startswith("find_") else w["packed"])._h
    ent = np.full(cap + GUARDS, GUARD64, dtype=np.uint64)
    dst = np.full(cap + GUARDS, GUARD8, dtype=np.uint8) if dist else None
    outs = [ent.ctypes.data if cap else None] + ([dst.ctypes.data if cap else None] if dist else [])
    c = ctypes.c_uint64(0xFFFFFFFF)
    L = smart_amd.lib()
    rc = getattr(L, "smartgpu_" + name)(pat.ctypes.data, m, *extra, handle, OFF, N - OFF, *outs, cap, ctypes.byref(c))
    return rc, int(c.value), ent, dst, L.smartgpu_last_error().decode()


def count_c(name, w):
    cname, _, kind, m, extra, _, _ = CALLS[name]
    pat = np.ascontiguousarray(w[kind], dtype=np.uint8)
    handle = (w["text"] if name.startswith("find_") else w["packed"])._h
    c = ctypes.c_uint64(0xFFFFFFFF)
    rc = getattr(smart_amd.lib(), "smartgpu_" + cname)(pat.ctypes.data, m, *extra, handle, OFF, N - OFF, ctypes.byref(c), None, None)
    assert rc == OK, (cname, rc)
    return int(c.value)


def guards_intact(ent, dst, cap):
    return bool((ent[cap:] == GUARD64).all()) and (dst is None or bool((dst[cap:] == GUARD8).all()))


@pytest.mark.parametrize("name,wide", CASES)
def test_the_contract_of_a_find(world, name, wide):
    w = world(wide, CALLS[name][3])
    want, wdist = expected(name, wide, w)
    count = len(want)
    print(name, "wide" if wide else "narrow", "count", count, "distances", np.bincount(wdist).tolist())
    base = OFF // 128 * 128
    spans = np.unique((want - base) // SPAN)
    assert count >= 3 and {0, 1, 2} <= set(spans.tolist()), (count, spans)  # the case itself: entries from three spans
    assert count_c(name, w) == count

    rc, c, ent, dst, _ = find_c(name, w, count)
    assert rc == OK and c == count, (rc, c, count)
    assert np.array_equal(ent[:count], want), (ent[:8], want[:8])
    if dst is not None:
        assert np.array_equal(dst[:count], wdist), (dst[:8], wdist[:8])
    assert guards_intact(ent, dst, count)

    rc, c, ent, dst, msg = find_c(name, w, count - 1)
    assert rc == ERR_NOMEM and c == count, (rc, c, count)
    assert "%d occurrences, room for %d" % (count, count - 1) in msg, msg
    assert guards_intact(ent, dst, count - 1)

    rc, c, ent, dst, msg = find_c(name, w, 0)
    assert rc == ERR_NOMEM and c == count, (rc, c, count)
    assert guards_intact(ent, dst, 0)
    assert count_c(name, w) == count
