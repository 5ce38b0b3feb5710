"""text_mis_scan / text_mis_find AT SIZE: many trips of the grid-stride tile loop with a ragged last one, and across byte 2^32.
The texts are a unit of U = 4109 bytes over all 256 values tiled on the device (Text.upload_tiled) to 2^32 + 2^28 + 77 bytes; what
the calls must return follows from the definition over three periods (tests/tiled_oracle.py, warm = m, span = m: starts).  U
is odd, so successive copies of the unit meet every phase of the 128-byte runs, the 8192-byte spans and the 32 KiB tiles.  Exact
equality.

Over 256 values the unit's own noise holds no occurrence at these k: unit() asserts, from the definition alone, that the
occurrences of a period are the planted copies with at most k substitutions, each at its own distance."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Text, find_mis, search_mis  # noqa: E402

from tiled_oracle import expected_tiled, expected_tiled_count, make_unit, tiled_slice  # noqa: E402

U = 4109
VALS = tuple(range(256))
CASES = {"m20-k2": (20, 2), "m64-k7": (64, 7)}
BEYOND = 2**32
BEYOND_N = 2**32 + 2**28 + 77
BEYOND_RANGE = (2**32 - 2**27 - 45, 2**28 + 1001)
PAST = 2**32 + 5            # the second range begins here: just past 2^32, mid-dword and mid-run
PAST_N = 2**20 + 333


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def by_definition(P, T, k):
    """(start positions int64, distances uint8) of P in T with at most k mismatches: tests/test_text_mis_gpu.py's, for bytes."""
    m = len(P)
    s = np.arange(0, len(T) - m + 1, dtype=np.int64)
    d = np.zeros(len(s), dtype=np.int32)
    for j in range(m):
        d += T[s + j] != P[j]
        keep = d <= k
        s, d = s[keep], d[keep]
    return s, d.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def unit(name):
    """(unit, P, k, planted): the unit with its planted copies of P — substitutions only; one across the unit's seam, one over
    byte 2^32 of a text of phase 0."""
    m, k = CASES[name]
    rng = np.random.default_rng(4000 + m)
    P = rng.integers(0, 256, m).astype(np.uint8)
    tile, planted = make_unit(VALS, P, k, U, 4100 + m, mixed=False)
    # (the inputs) a period's occurrences are the planted copies within k, each at its own distance, and nothing else
    pos, dist = by_definition(P, tiled_slice(tile, 0, 3 * U), k)
    second = (pos >= U) & (pos < 2 * U)
    near = sorted((a, d) for a, _, d in planted if d <= k)
    assert len(near) >= 6 and any(d > k for _, _, d in planted) and {0, k} <= {d for _, d in near}
    assert sorted(zip((pos[second] - U).tolist(), dist[second].tolist())) == near
    tile.setflags(write=False)
    return tile, P, k, planted


def reference(name, phase):
    tile, P, k, _ = unit(name)

    def ref(off, length):
        pos, dist = by_definition(P, tiled_slice(tile, off, length, phase), k)
        return pos + off, dist
    return ref


def check(text, name, phase, lo, hi):
    tile, P, k, _ = unit(name)
    m = len(P)
    ref = reference(name, phase)
    wpos, wdist = expected_tiled(ref, U, lo, hi, m, m)
    assert len(wpos) == expected_tiled_count(ref, U, lo, hi, m, m) > 0
    got = search_mis(P, text, k, off=lo, n=hi - lo)
    assert got == len(wpos), (name, lo, hi, got, len(wpos))
    pos, dist = find_mis(P, text, k, off=lo, n=hi - lo, cap=len(wpos))
    assert len(pos) == len(wpos) and np.array_equal(pos, wpos), (name, lo, hi, first_difference(pos, wpos))
    assert np.array_equal(dist, wdist), (name, lo, hi, first_difference(dist, wdist))
    return wpos.astype(np.int64), wdist


def first_difference(a, b):
    at = int(np.flatnonzero(a != b)[0]) if len(a) == len(b) else -1
    return at, len(a), len(b)


def test_across_2_to_the_32():
    """Phase 0: make_unit's mark covers byte 2^32.  The COUNT is compared over the whole text — 2^17 + 2^13 + 1 tiles, well
    over a hundred trips of every workgroup's tile loop, the last tile 77 bytes —; the find's positions and distances over a
    range of 2^28 + 1001 bytes on both sides of 2^32."""
    for name in CASES:
        tile, P, k, _ = unit(name)
        m = len(P)
        text = Text.upload_tiled(tile, BEYOND_N)
        try:
            assert len(text) == BEYOND_N
            for off in (BEYOND - 4096, BEYOND_N - 4096):
                assert np.array_equal(text.read(off, 4096), tiled_slice(tile, off, 4096))
            whole = expected_tiled_count(reference(name, 0), U, 0, BEYOND_N, m, m)
            assert whole > BEYOND_N // U * 6
            got = search_mis(P, text, k)
            assert got == whole, (name, got, whole)
            lo, ln = BEYOND_RANGE
            wpos, _ = check(text, name, 0, lo, lo + ln)
            assert wpos[0] < BEYOND < wpos[-1]
            # an occurrence whose window contains byte 2^32 and begins before it
            assert ((wpos < BEYOND) & (wpos + m > BEYOND)).any()
        finally:
            text.free()


def test_a_range_that_begins_just_past_2_to_the_32():
    """The phase puts an exact copy's first byte on byte 2^32 + 5.  The range that begins there reports it as its first entry,
    though the lane that owns its end starts fresh at the range's first byte, not m - 1 before its run; the range that begins one
    byte later does not report it, and no end among the range's first m - 1 is an occurrence."""
    for name in CASES:
        tile, P, k, planted = unit(name)
        m = len(P)
        a0 = next(a for a, _, d in planted if d == 0 and a + m <= U)
        phase = (a0 - PAST) % U
        text = Text.upload_tiled(tile, BEYOND_N, phase)
        try:
            assert np.array_equal(text.read(PAST, m), P)  # (the inputs)
            wpos, wdist = check(text, name, phase, PAST, PAST + PAST_N)
            assert wpos[0] == PAST and wdist[0] == 0
            wpos, _ = check(text, name, phase, PAST + 1, PAST + PAST_N)
            assert wpos[0] > PAST + m
            # and one that ends with the text: the ragged last tile, a range of less than a run before it
            wpos, _ = check(text, name, phase, BEYOND_N - 3 * U - 50, BEYOND_N)
            assert wpos[-1] > BEYOND_N - U - m
        finally:
            text.free()
