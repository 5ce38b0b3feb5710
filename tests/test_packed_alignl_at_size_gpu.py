"""planes_editl_align ACROSS SYMBOL 2^32: the 64-bit addressing of the wave's window and of the starts it returns.  The text is
a unit of U = 8209 symbols over four values (tests/tiled_oracle.py: make_unit, with copies of a 150-symbol pattern that carry
0 .. k + 1 mixed edits, one of them over symbol 2^32) tiled on the device to 2^32 + 2^28 + 77 symbols (Text.upload_tiled:
nothing of that size crosses the bus) and packed there; the byte text is freed before the calls.  A few thousand ends on both
sides of 2^32 — those of pfind_editl over a range of twelve periods around it, and EVERY end within 1000 symbols of it — and a
second range that BEGINS beyond 2^32, at the first symbol of an exact copy of the pattern, and lists the ends off .. off + m + k,
whose bands are clipped beyond 2^32 (one of them IS an occurrence).  What the calls must return comes from the by-definition
oracle (align_manyl of tests/test_text_alignl.py) on tiled_slice over three periods: a band reads at most m + k symbols, so an
end e that lies m + k - 1 or more behind its range's first symbol is mapped to e mod U + U and its start shifted back; the few
ends nearer to the range's first symbol are computed in place, with the range's off.  Exact equality."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import PackedText, Text, palign_editl, pfind_editl  # noqa: E402

from test_packed_align import NONE_DIST  # noqa: E402
from test_packed_edit import byte_accepts  # noqa: E402
from test_text_alignl import WORDS, align_manyl  # noqa: E402
from tiled_oracle import make_unit, tiled_slice  # noqa: E402

U = 8209
M, K = 150, 10
ACGT = (65, 67, 71, 84)
BEYOND = 2**32
BEYOND_N = 2**32 + 2**28 + 77
RANGE = (BEYOND - 6 * U - 45, 12 * U + 1001)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


@functools.lru_cache(maxsize=None)
def unit():
    rng = np.random.default_rng(9050)
    P = np.asarray(ACGT, dtype=np.uint8)[rng.integers(0, 4, M)]
    tile, planted = make_unit(ACGT, P, K, U, 9051, mixed=True)
    assert any(d <= K for _, _, d in planted) and any(d > K for _, _, d in planted)
    a0 = next(a for a, ln, d in planted if d == 0 and a + ln <= U)  # an exact copy that does not wrap the unit's seam
    assert np.array_equal(tile[a0:a0 + M], P)
    tile.setflags(write=False)
    return tile, P, BEYOND + 1 + (a0 - BEYOND - 1) % U  # the first text position beyond 2^32 at which that copy begins


def expected(ends, off):
    """(starts, distances, ops) of the ends (any order) of the range that begins at off, by the oracle on three periods."""
    tile, P, _ = unit()
    accepts = byte_accepts(P)
    ends = np.asarray(ends, dtype=np.int64)
    starts = np.zeros(len(ends), dtype=np.uint64)
    dist = np.zeros(len(ends), dtype=np.uint8)
    ops = np.zeros((len(ends), WORDS), dtype=np.uint64)
    head = ends - off + 1 < M + K  # bands that the range's first symbol clips: in place
    for part, base, o in ((head, off - U, U), (~head, None, 0)):
        if not part.any():
            continue
        if base is None:  # periodic: one representative per residue, in the second of three periods
            S = tiled_slice(tile, 0, 3 * U)
            local = ends[part] % U + U
        else:
            S = tiled_slice(tile, base, 3 * U)
            local = ends[part] - base
        uniq, inverse = np.unique(local, return_inverse=True)
        s, d, w = (np.concatenate(x) for x in zip(*(align_manyl(M, accepts, S, uniq[a:a + 512], K, o) for a in range(0, len(uniq), 512))))
        s_all, d_all, w_all = s[inverse], d[inverse], w[inverse]
        moved = np.where(d_all != NONE_DIST, (s_all.astype(np.int64) + ends[part] - local).astype(np.uint64), s_all)
        starts[part], dist[part], ops[part] = moved, d_all, w_all
    return starts, dist, ops


def first_difference(a, b, ends):
    at = int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])
    return at, int(ends[at]), int(a[at]), int(b[at])


def test_ends_on_both_sides_of_2_to_the_32_and_bands_clipped_beyond_it():
    tile, P, CLIP_OFF = unit()
    lo, ln = RANGE
    near = np.arange(BEYOND - 1000, BEYOND + 1000, dtype=np.uint64)
    clip_ends = np.arange(CLIP_OFF, CLIP_OFF + M + K + 1, dtype=np.uint64)
    cs, cd, co = expected(clip_ends, CLIP_OFF)
    # (the inputs) a clipped band that is an occurrence — the copy itself, start CLIP_OFF, distance 0 — and clipped ones that are none
    assert BEYOND < CLIP_OFF <= BEYOND + U and (int(cs[M - 1]), int(cd[M - 1])) == (CLIP_OFF, 0) and (cd == NONE_DIST).any()
    assert (cs[cd != NONE_DIST] >= CLIP_OFF).all()
    text = Text.upload_tiled(tile, BEYOND_N)
    try:
        pt = PackedText.pack(text)
    finally:
        text.free()
    with pt:
        assert len(pt) == BEYOND_N and pt.planes == 2
        for off in (BEYOND - 4096, BEYOND_N - 4096):
            assert np.array_equal(pt.read(off, 4096), tiled_slice(tile, off, 4096))
        fends, fdist, cnt = pfind_editl(P, pt, K, off=lo, n=ln, cap=1 << 20)
        assert cnt == len(fends) > 0 and int(fends[0]) < BEYOND <= int(fends[-1])
        # an occurrence whose match contains symbol 2^32 (make_unit's mark): it ends at most m + k - 1 symbols behind it
        assert ((fends >= BEYOND) & (fends < BEYOND + M + K)).any()
        ends = np.concatenate([fends, near])
        ws, wd, wo = expected(ends, lo)
        assert np.array_equal(wd[:len(fends)], fdist)  # the oracle and the find agree on the distances before the align call is asked
        assert (wd[len(fends):] == NONE_DIST).any() and len(ends) >= 2000
        starts, dist, ops = palign_editl(P, pt, K, ends, off=lo, n=ln)
        assert np.array_equal(dist, wd), first_difference(dist, wd, ends)
        assert np.array_equal(starts, ws), first_difference(starts, ws, ends)
        assert np.array_equal(ops, wo), first_difference((ops != wo).any(axis=1), np.zeros(len(ends), dtype=bool), ends)
        hit = dist != NONE_DIST
        assert (starts[hit] < BEYOND).any() and (starts[hit] >= BEYOND).any() and ((starts[hit] < BEYOND) & (ends[hit] >= BEYOND)).any()
        s2, d2, o2 = palign_editl(P, pt, K, ends, off=lo, n=ln, ops=False)
        assert o2 is None and np.array_equal(s2, ws) and np.array_equal(d2, wd)
        # the range that begins beyond 2^32
        for with_ops in (True, False):
            s, d, o = palign_editl(P, pt, K, clip_ends, off=CLIP_OFF, n=4096, ops=with_ops)
            assert np.array_equal(d, cd), (with_ops, first_difference(d, cd, clip_ends))
            assert np.array_equal(s, cs), (with_ops, first_difference(s, cs, clip_ends))
            assert (o is None) if not with_ops else np.array_equal(o, co), with_ops
