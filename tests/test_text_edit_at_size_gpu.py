"""text_edit_scan / text_edit_find AT SIZE: past one sweep of the grid, and across byte 2^32.  The texts are a unit of
U = 4109 bytes over all 256 values tiled on the device (Text.upload_tiled, phase 0); what the calls must return follows from
the by-definition oracle over three periods (tests/tiled_oracle.py, warm = m + k, span = 1: ends).  U is odd, so successive
copies of the unit meet every phase of the 128-byte runs, the 8192-byte spans and the 32 KiB tiles.  Exact equality.

Over 256 values the unit's own noise holds no occurrence at these k: unit() asserts, from the reference alone, that every
expected end of a period lies within k bytes of the end of a planted copy with at most k edits, and that each such copy is
found."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Text, find_edit, search_edit  # noqa: E402

from test_packed_edit import byte_accepts, edit_occurrences  # noqa: E402
from tiled_oracle import expected_tiled, expected_tiled_count, make_unit, tiled_slice  # noqa: E402

U = 4109
VALS = tuple(range(256))
CASES = {"m20-k2": (20, 2), "m64-k7": (64, 7)}
SWEEP_N = 2**26 + 2**25 + 77          # more than 8 workgroups x 256 CUs x 32 KiB: every workgroup makes a second trip, the last is ragged
BEYOND = 2**32
BEYOND_N = 2**32 + 2**28 + 77
BEYOND_RANGE = (2**32 - 2**27 - 45, 2**28 + 1001)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


@functools.lru_cache(maxsize=None)
def unit(name):
    """(unit, P, k, ref): the unit with its planted copies of P — one across the unit's seam, one over byte 2^32 of a text of
    phase 0 —, and ref(off, length), the oracle on bytes [off, off + length) of the tiled text alone."""
    m, k = CASES[name]
    rng = np.random.default_rng(3000 + m)
    P = rng.integers(0, 256, m).astype(np.uint8)
    tile, planted = make_unit(VALS, P, k, U, 3100 + m, mixed=True)

    def ref(off, length):
        pos, dist = edit_occurrences(m, byte_accepts(P), tiled_slice(tile, off, length), k)
        return pos.astype(np.int64) + off, dist

    # (the inputs) the reference finds the planted copies and nothing else
    pos, dist = ref(0, 3 * U)
    second = pos[(pos >= U) & (pos < 2 * U)] - U
    near = [c for c in planted if c[2] <= k]
    assert len(near) >= 6 and any(c[2] > k for c in planted)
    ends = np.asarray([(a + ln - 1) % U for a, ln, _ in near], dtype=np.int64)
    gap = np.abs((second[:, None] - ends[None, :] + U // 2) % U - U // 2)
    assert (gap.min(axis=1) <= k).all(), "an occurrence that no planted copy explains"
    assert (gap.min(axis=0) == 0).all(), "a planted copy the reference does not find"
    tile.setflags(write=False)
    return tile, P, k, ref


def check(text, name, lo, hi):
    tile, P, k, ref = unit(name)
    m = len(P)
    wends, wdist = expected_tiled(ref, U, lo, hi, m + k, 1)
    assert len(wends) == expected_tiled_count(ref, U, lo, hi, m + k, 1) > 0
    got = search_edit(P, text, k, off=lo, n=hi - lo)
    assert got == len(wends), (name, lo, hi, got, len(wends))
    ends, dist = find_edit(P, text, k, off=lo, n=hi - lo, cap=len(wends))
    assert len(ends) == len(wends) and np.array_equal(ends, wends), (name, lo, hi, first_difference(ends, wends))
    assert np.array_equal(dist, wdist), (name, lo, hi, first_difference(dist, wdist))
    return wends


def first_difference(a, b):
    at = int(np.flatnonzero(a != b)[0]) if len(a) == len(b) else -1
    return at, len(a), len(b)


def test_a_second_sweep_of_the_grid():
    """2^26 + 2^25 + 77 bytes: more tiles than the largest grid has workgroups, so the tile loop's second trip (and with it the
    barriers between two tiles) runs in every workgroup, and the last trip is ragged.  One dword and two; count and find."""
    for name in CASES:
        text = Text.upload_tiled(unit(name)[0], SWEEP_N)
        try:
            assert len(text) == SWEEP_N
            wends = check(text, name, 0, SWEEP_N)
            assert int(wends[-1]) > SWEEP_N - U
        finally:
            text.free()


def test_across_2_to_the_32():
    """2^32 + 2^28 + 77 bytes, phase 0: make_unit's mark covers byte 2^32.  Only a sub-range around it is searched; the count,
    and the find's ends and distances on both sides of 2^32, are compared in full."""
    for name in CASES:
        tile, P, k, ref = unit(name)
        text = Text.upload_tiled(tile, BEYOND_N)
        try:
            assert len(text) == BEYOND_N
            for off in (BEYOND - 4096, BEYOND_N - 4096):
                assert np.array_equal(text.read(off, 4096), tiled_slice(tile, off, 4096))
            lo, ln = BEYOND_RANGE
            wends = check(text, name, lo, lo + ln).astype(np.int64)
            assert wends[0] < BEYOND < wends[-1]
            # an occurrence whose match contains byte 2^32: it ends at most m + k - 1 bytes behind it
            assert ((wends >= BEYOND) & (wends < BEYOND + len(P) + k)).any()
        finally:
            text.free()
