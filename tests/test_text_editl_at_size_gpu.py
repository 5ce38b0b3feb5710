"""text_editl_scan / text_editl_find AT SIZE: past one sweep of the grid, and across byte 2^32.  The texts are a unit of
U = 8209 bytes over all 256 values tiled on the device (Text.upload_tiled, phase 0) — tests/test_text_edit_at_size_gpu.py's
unit of 4109 bytes has no room for ten copies of a 256-byte pattern —; what the calls must return follows from the
by-definition oracle over three periods (tests/tiled_oracle.py, warm = m + k, span = 1: ends).  U is odd, so successive copies
of the unit meet every phase of the 128-byte pieces, the 512-byte runs, the 32 KiB of a wave and the 128 KiB super-tiles.
Exact equality.

Over 256 values the unit's own noise holds no occurrence at these k: unit() asserts, from the reference alone, that every
expected end of a period lies within k bytes of the end of a planted copy with at most k edits, and that each such copy is
found."""
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Text, find_editl, search_editl, sources  # noqa: E402

from test_packed_edit import byte_accepts, edit_occurrences  # noqa: E402
from tiled_oracle import expected_tiled, expected_tiled_count, make_unit, tiled_slice  # noqa: E402

U = 8209
VALS = tuple(range(256))
CASES = {"m100-k7": (100, 7), "m256-k31": (256, 31)}
# what k_teditl.hip chose (teditl_host.hpp, teditl.hpp; test_the_restated_geometry_is_the_kernels): a lane's run, its piece,
# the lanes of a workgroup, and the LDS that decides how many workgroups a CU holds
RUN, PIECE, LANES = 512, 128, 256
SUPER = LANES * RUN
LDS_CU = 160 * 1024


def words(m):
    return 2 if m <= 64 else 4 if m <= 128 else 8


def workgroups_per_cu(m):
    return LDS_CU // (128 + 1024 * words(m) + LANES * (PIECE + 4))


NUM_CUS = 256  # an MI355X
# more super-tiles than the largest grid has workgroups: some workgroups make a second trip through the super-tile loop (and
# with it through the barriers between two super-tiles), the last super-tile is ragged
SWEEP_N = NUM_CUS * max(workgroups_per_cu(m) for m, k in CASES.values()) * SUPER + 2**26 + 77
BEYOND = 2**32
BEYOND_N = 2**32 + 2**28 + 77
BEYOND_RANGE = (2**32 - 2**27 - 45, 2**28 + 1001)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def test_the_restated_geometry_is_the_kernels():
    host = open(os.path.join(sources.CSRC, "teditl_host.hpp")).read()
    assert re.search(r"constexpr uint32_t kTEditlRun = %d;" % RUN, host)
    assert re.search(r"constexpr uint32_t kTEditlPiece = %d;" % PIECE, host)
    assert re.search(r"constexpr uint32_t kTEditlLanes = %d;" % LANES, host)
    head = open(os.path.join(sources.CSRC, "teditl.hpp")).read()
    assert re.search(r"constexpr uint32_t kTEditlLdsCu = 160u \* 1024u;", head)
    assert re.search(r"kTEditlRowBytes = kTEditlPiece \+ 4\b", head) and re.search(r"kTEditlMasksOff = 128;", head)
    assert re.search(r"teditl_rows_off\(int words\) \{ return kTEditlMasksOff \+ 1024u \* words; \}", head)
    assert re.search(r"static_assert\(teditl_wgs\(2\) == %d && teditl_wgs\(4\) == %d && teditl_wgs\(8\) == %d" %
                     (workgroups_per_cu(64), workgroups_per_cu(128), workgroups_per_cu(256)), head)
    assert SWEEP_N > NUM_CUS * workgroups_per_cu(100) * SUPER and SWEEP_N % SUPER != 0 and SWEEP_N % RUN != 0


@functools.lru_cache(maxsize=None)
def unit(name):
    """(unit, P, k, ref): the unit with its planted copies of P — one across the unit's seam, one over byte 2^32 of a text of
    phase 0 —, and ref(off, length), the oracle on bytes [off, off + length) of the tiled text alone."""
    m, k = CASES[name]
    rng = np.random.default_rng(6000 + m)
    P = rng.integers(0, 256, m).astype(np.uint8)
    tile, planted = make_unit(VALS, P, k, U, 6100 + m, mixed=True)

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
    got = search_editl(P, text, k, off=lo, n=hi - lo)
    assert got == len(wends), (name, lo, hi, got, len(wends))
    ends, dist = find_editl(P, text, k, off=lo, n=hi - lo, cap=len(wends))
    assert len(ends) == len(wends) and np.array_equal(ends, wends), (name, lo, hi, first_difference(ends, wends))
    assert np.array_equal(dist, wdist), (name, lo, hi, first_difference(dist, wdist))
    return wends


def first_difference(a, b):
    at = int(np.flatnonzero(a != b)[0]) if len(a) == len(b) else -1
    return at, len(a), len(b)


def test_a_second_sweep_of_the_grid():
    """More super-tiles than the largest grid has workgroups, and a ragged one.  Four dwords and eight; count and find."""
    for name in CASES:
        text = Text.upload_tiled(unit(name)[0], SWEEP_N)
        try:
            assert len(text) == SWEEP_N
            wends = check(text, name, 0, SWEEP_N)
            assert int(wends[-1]) > SWEEP_N - U
        finally:
            text.free()


def test_across_2_to_the_32():
    """2^32 + 2^28 + 77 bytes, phase 0: make_unit's mark covers byte 2^32.  Only a sub-range around it is searched, unaligned at
    both ends; the count, and the find's ends and distances on both sides of 2^32, are compared in full."""
    for name in CASES:
        tile, P, k, ref = unit(name)
        text = Text.upload_tiled(tile, BEYOND_N)
        try:
            assert len(text) == BEYOND_N
            for off in (BEYOND - 4096, BEYOND_N - 4096):
                assert np.array_equal(text.read(off, 4096), tiled_slice(tile, off, 4096))
            lo, ln = BEYOND_RANGE
            assert lo % PIECE != 0 and (lo + ln) % PIECE != 0
            wends = check(text, name, lo, lo + ln).astype(np.int64)
            assert wends[0] < BEYOND < wends[-1]
            # an occurrence whose match contains byte 2^32: it ends at most m + k - 1 bytes behind it
            assert ((wends >= BEYOND) & (wends < BEYOND + len(P) + k)).any()
        finally:
            text.free()
