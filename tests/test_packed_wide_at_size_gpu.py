"""planes3_scan and planes3_find AT SIZE: one three-plane text of 2^32 + 2^28 + 77 symbols over five values — several trips
of the grid-stride loop (the launchers cap the grid; the kernels walk the rest with `cw += stride`), a ragged last one, and
positions beyond 32 bits.  The text is a unit of U = 2^18 + 13 symbols tiled on the device (Text.upload_tiled) and packed with
wide=True, as tests/test_packed_at_size_gpu.py builds its texts; what a call must return over any range follows from the
by-definition reference of tests/test_packed_wide_gpu.py over three periods (tests/tiled_oracle.py).  Every comparison is
exact equality."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import PackedText, Text, pfind, pfind_mis, psearch, psearch_mis  # noqa: E402

from test_packed_wide_gpu import ACGNT, by_definition, sets_of  # noqa: E402
from tiled_oracle import expected_tiled, expected_tiled_count, make_unit, tiled_slice  # noqa: E402

N = 2**32 + 2**28 + 77
U = 2**18 + 13
BEYOND = 2**32
M, K = 20, 2
SUB_RANGE = (2**32 - 2**27 - 45, 2**28 + 1001)  # straddles 2^32, unaligned


@functools.lru_cache(maxsize=None)
def unit():
    """(unit, pattern): U uniform symbols over ACGNT with copies of a 20-symbol pattern at 0, 1, 1, 2, 2 and 3 substitutions,
    one across the unit's seam and one over symbol 2^32 of the text (tiled_oracle.make_unit)."""
    rng = np.random.default_rng(7300)
    P = np.asarray(ACGNT, dtype=np.uint8)[rng.integers(0, 5, M)]
    u, planted = make_unit(ACGNT, P, K, U, 7301)
    assert len(planted) >= 6 and set(np.unique(u).tolist()) == set(ACGNT)
    return u, P


def ref(k):
    u, P = unit()

    def run(off, length):
        pos, dist = by_definition(sets_of(P, ACGNT), tiled_slice(u, off, length), ACGNT, k)
        return pos.astype(np.int64) + off, dist
    return run


@pytest.fixture(scope="module")
def packed():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()
    u, _ = unit()
    text = Text.upload_tiled(u, N)
    try:
        pt = PackedText.pack(text, wide=True)
    finally:
        text.free()
    assert len(pt) == N and pt.planes == 3 and pt.symbols() == list(ACGNT)
    for off in (0, BEYOND - 4096, N - 4096):
        assert np.array_equal(pt.read(off, 4096), tiled_slice(u, off, 4096)), off
    yield pt
    pt.free()


def test_exact_count_over_the_whole_text(packed):
    _, P = unit()
    want = expected_tiled_count(ref(0), U, 0, N, M, M)
    assert want >= N // U  # the exact copy of every period
    assert psearch(P, packed)[0] == want
    assert pfind(P, packed, cap=0) == (None, want)


def test_k2_count_over_the_whole_text(packed):
    _, P = unit()
    want = expected_tiled_count(ref(K), U, 0, N, M, M)
    assert want >= 5 * (N // U) > expected_tiled_count(ref(0), U, 0, N, M, M)
    assert psearch_mis(P, packed, K)[0] == want


def test_find_over_a_sub_range_that_straddles_2_to_the_32(packed):
    _, P = unit()
    lo, ln = SUB_RANGE
    for k in (0, K):
        wpos, wdist = expected_tiled(ref(k), U, lo, lo + ln, M, M)
        assert len(wpos) > 0 and int(wpos[0]) < BEYOND < int(wpos[-1])
        if k == 0:
            pos, cnt = pfind(P, packed, off=lo, n=ln, cap=len(wpos))
        else:
            pos, dist, cnt = pfind_mis(P, packed, k, off=lo, n=ln, cap=len(wpos))
            assert dist.dtype == np.uint8 and np.array_equal(dist, wdist)
            assert ((wpos <= BEYOND) & (wpos + M > BEYOND)).any()  # a window that contains symbol 2^32
        assert cnt == len(wpos) and pos.dtype == np.uint64 and np.array_equal(pos, wpos), k
