"""hor_multi_scan builds its tails and its skip table from rows that carry each pattern's last bytes by value
(multi.hpp: kTailRow, tail_fill, tail_at), and asks for its first tile before it builds them.  What that can get wrong:

* the row: m = 65, 66, 67 are the two sides of the 65 bytes a row stores (a row holds the whole pattern up to 65), 100 and
  300 lie far beyond; m = 8, 17 against 18, 65 ... are the two sides of "completed in memory" (m - 1 > 16), where the
  blob pointers are still read;
* the first tile, requested before the table exists: texts shorter than a tile (5 000 bytes) and of two tiles and a
  part (40 000), each searched from offset 0 and from offset 4 099;
* the table: a pattern ending on the last byte of a tile and one ending on the first byte of the next, two identical
  patterns, two patterns with one last gram, and two whose last grams (10, 20) and (65, 33) differ but share slot 390;
  both grams also stand in the text every 97 bytes without the rest of a pattern, so that slot hits that are no gram
  hits occur.

Groups of 8, 3 and 2.  Every count against the oracle's brute force and against the same launches under
smartgpu_coalesce(0), one pass per group.  Bit-exact.  The helpers are those of tests/test_coalesce_gram_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_coalesce_gram_gpu import TILE, Case, groups_of_eight, need_gpu, slot, streaming  # noqa: E402,F401

N_BIG, N_SMALL = 40000, 5000
SEED = 0x5EED7A11
GRAM_A, GRAM_B = (10, 20), (65, 33)


def build(po, m, n, off):
    """The first of the texts edit(.., salt) all of whose patterns take hor_scan's streaming form (nearly always salt 0)."""
    for salt in range(16):
        T, pats = edit(po, m, n, off, salt)
        if all(streaming(P) for P in pats):
            return T, pats
    raise AssertionError("no text with eight streaming patterns: m %d n %d off %d" % (m, n, off))


def edit(po, m, n, off, salt):
    """-> (T, pats): a rand256 text of n bytes, edited, and eight patterns cut from T[off:] AFTER the edits:
    0 and 1 identical; 2 with 0's last gram; 3 ending in GRAM_A, 4 in GRAM_B; 5 ending on the last byte of the first
    tile, 6 on the first byte of the third (where the text has them); 7 as the text gives it."""
    T = po.gen_text(SEED + 1000 * salt + m, 256, 0, n).copy()
    lo, hi = off, n - m - 8  # start positions; the last 8 bytes of the text stay free for two bare grams
    for x in range(lo + m + 1, hi, 97):  # the two grams without their patterns, alternating
        T[x:x + 2] = GRAM_A if (x // 97) % 2 else GRAM_B
    T[n - 6:n - 4] = GRAM_A
    T[n - 4:n - 2] = GRAM_B
    step = (hi - lo) // 7
    assert step >= 2
    ks = [lo + j * step for j in range(8)]
    if n > 2 * TILE + 1:
        ks[5], ks[6] = TILE - 1 - (m - 1), 2 * TILE - (m - 1)
    assert len({k + m for k in ks}) == 8 and min(ks) >= lo and max(ks) <= hi
    T[ks[3] + m - 2:ks[3] + m] = GRAM_A
    T[ks[4] + m - 2:ks[4] + m] = GRAM_B
    T[ks[2] + m - 2:ks[2] + m] = T[ks[0] + m - 2:ks[0] + m]
    pats = [T[k:k + m].copy() for k in ks]
    pats[1] = pats[0].copy()
    assert len({bytes(P) for P in pats}) == 7
    assert tuple(pats[3][m - 2:]) == GRAM_A and tuple(pats[4][m - 2:]) == GRAM_B and np.array_equal(pats[2][m - 2:], pats[0][m - 2:])
    return T, pats


def test_the_two_grams_share_a_slot():
    assert slot(*GRAM_A) == slot(*GRAM_B) == 390 and GRAM_A != GRAM_B


@pytest.mark.parametrize("off", (0, 4099))
@pytest.mark.parametrize("n", (N_SMALL, N_BIG))
@pytest.mark.parametrize("m", (8, 17, 18, 65, 66, 67, 100, 300))
def test_tails_and_table_from_the_argument_rows(oracle, m, n, off):
    T, pats = build(oracle, m, n, off)
    c = Case(oracle, T, pats, off=off, n=n - off)
    assert min(c.want) >= 1 and c.want[0] == c.want[1]
    c.check()               # eight
    c.check((0, 1))         # two identical patterns
    c.check((3, 4))         # two last grams in one slot
    c.check((2, 0, 6))      # one last gram twice, and the pattern on the first byte of a tile
    c.check((5, 6, 3))      # the patterns at the tile boundary
    c.free()
