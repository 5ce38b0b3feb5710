"""smartgpu_find_batch64 past 2^32 bytes: one tiled text (Text.upload_tiled) from a unit of 2^20 + 7 bytes of rand128, 90
patterns of m = 20 cut from the unit.  64-bit positions, entries above 2^32 << 18, and several trips of the kernel's
grid-stride loop.  What a range must return follows from the unit (tests/tiled_oracle.py).

The text is 2^32 + 2^21 + 2^20 + 77 bytes: the range the sub-range test asks for, [2^32 - 2^21 - 45, +2^22 + 1001), ends at
2^32 + 2^21 + 956, which a text of 2^32 + 2^20 + 77 bytes does not hold (the call refuses a range outside the text), so the
text is 2^21 bytes longer than that and the range is kept as it is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Text, engine  # noqa: E402
from tiled_oracle import expected_tiled, tiled_slice  # noqa: E402

U = 2**20 + 7
N = 2**32 + 2**21 + 2**20 + 77
M = 20
K = 90


@pytest.fixture(scope="module")
def big():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()
    rng = np.random.default_rng(0xF1BA7C64)
    unit = rng.integers(0, 128, U, dtype=np.uint8)
    cuts = rng.integers(0, U - M, K - 1).tolist() + [U - M // 2]  # the last pattern wraps the unit's seam
    pats = [tiled_slice(unit, c, M) for c in cuts]
    text = Text.upload_tiled(unit, N)
    assert len(text) == N
    yield unit, pats, text
    text.free()


def test_positions_across_2_to_the_32(big):
    unit, pats, text = big
    lo, ln = 2**32 - 2**21 - 45, 2**22 + 1001
    hi = lo + ln
    hay = tiled_slice(unit, lo, 3 * U).tobytes()  # the three periods the oracle computes, once for all patterns

    def ref_of(P):
        needle = P.tobytes()

        def ref(off, length):
            assert off == lo and length <= len(hay)
            found, s = [], hay.find(needle)
            while s != -1 and s + M <= length:
                found.append(lo + s)
                s = hay.find(needle, s + 1)
            return np.array(found, dtype=np.int64)
        return ref

    want = [expected_tiled(ref_of(P), U, lo, hi, warm=M, span=M)[0] for P in pats]
    assert all(len(w) >= 4 for w in want) and any(int(w[-1]) > 2**32 for w in want) and any(int(w[0]) < 2**32 for w in want)
    lists, counts = engine.find_batch(pats, text, lo, ln)
    assert counts.tolist() == [len(w) for w in want]
    for k, (got, w) in enumerate(zip(lists, want)):
        assert np.array_equal(got, w), (k, got[:4], w[:4])


def test_whole_text_counts(big):
    unit, pats, text = big
    counts = engine.search_batch("hor", pats, text, per_pattern_times=False)[0]
    total = int(counts.sum())
    assert total >= K * (N // U)
    lists, got = engine.find_batch(pats, text, cap=total)
    assert got.tolist() == counts.tolist()
    for k, pos in enumerate(lists):
        assert len(pos) == int(counts[k]) and (np.diff(pos.astype(np.int64)) > 0).all(), k
        assert int(pos[-1]) > 2**32 and np.array_equal(tiled_slice(unit, int(pos[-1]), M), pats[k]), k
    assert engine.find_batch(pats, text, cap=total - 1)[0] is None
