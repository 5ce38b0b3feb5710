"""text_edit_align ACROSS BYTE 2^32.  The text is the 4109-byte unit of tests/test_text_edit_at_size_gpu.py tiled on the device
to 2^32 + 2^28 + 77 bytes (Text.upload_tiled: nothing of that size crosses the bus); the ends are those of find_edit over that
file's BEYOND_RANGE, on both sides of 2^32, and a second range BEGINS at 2^32 + 5 and lists the ends off .. off + m + k, whose
walks are clipped beyond 2^32.  What the calls must return comes from the by-definition oracle (align_many of
tests/test_packed_align.py) on tiled_slice over three periods: a walk reads at most m + k bytes, so an end e that lies
m + k - 1 or more behind its range's first byte is mapped to e mod U + U and its start shifted back; the few ends nearer to the
range's first byte are computed in place, with the range's off.  Exact equality.

The text's PHASE is chosen per case so that the period's nearest occurrence ends m - 1 bytes behind 2^32 + 5: a clipped walk that
IS an occurrence (with phase 0 the copy that covers byte 2^32 is cut by the second range and no clipped walk is one)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import Text, align_edit, find_edit  # noqa: E402

from test_packed_align import NONE_DIST, align_many  # noqa: E402
from test_packed_edit import byte_accepts  # noqa: E402
from test_text_edit_at_size_gpu import BEYOND, BEYOND_N, BEYOND_RANGE, CASES, U, unit  # noqa: E402
from tiled_oracle import tiled_slice  # noqa: E402

CLIP_OFF = BEYOND + 5


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def phase_for(name):
    """The phase that puts the end of the period's nearest occurrence (the first of them) at text byte CLIP_OFF + m - 1."""
    tile, P, k, ref = unit(name)
    pos, dist = ref(0, 3 * U)
    second = (pos >= U) & (pos < 2 * U)
    c_end = int(pos[second][np.argmin(dist[second])]) - U
    return (c_end - (CLIP_OFF + len(P) - 1)) % U


def expected(name, phase, ends, off):
    """(starts, distances, ops) of the ends (any order) of the range that begins at off, by the oracle on three periods."""
    tile, P, k, _ = unit(name)
    m = len(P)
    accepts = byte_accepts(P)
    ends = np.asarray(ends, dtype=np.int64)
    starts = np.zeros(len(ends), dtype=np.uint64)
    dist = np.zeros(len(ends), dtype=np.uint8)
    ops = np.zeros((len(ends), 3), dtype=np.uint64)
    head = ends - off + 1 < m + k  # walks that the range's first byte clips: in place
    for part, base, o in ((head, off - U, U), (~head, None, 0)):
        if not part.any():
            continue
        if base is None:  # periodic: one representative per residue, in the second of three periods
            S = tiled_slice(tile, 0, 3 * U, phase)
            local = ends[part] % U + U
        else:
            S = tiled_slice(tile, base, 3 * U, phase)
            local = ends[part] - base
        uniq, inverse = np.unique(local, return_inverse=True)
        s, d, w = align_many(m, accepts, S, uniq, k, o)
        s_all, d_all, w_all = s[inverse], d[inverse], w[inverse]
        moved = np.where(d_all != NONE_DIST, (s_all.astype(np.int64) + ends[part] - local).astype(np.uint64), s_all)
        starts[part], dist[part], ops[part] = moved, d_all, w_all
    return starts, dist, ops


@pytest.mark.parametrize("name", list(CASES))
def test_ends_on_both_sides_of_2_to_the_32_and_walks_clipped_beyond_it(name):
    tile, P, k, ref = unit(name)
    m = len(P)
    phase = phase_for(name)
    lo, ln = BEYOND_RANGE
    # (the inputs, from the reference alone) the clipped range: ends off .. off + m + k, at least one clipped walk is an occurrence
    clip_ends = np.arange(CLIP_OFF, CLIP_OFF + m + k + 1, dtype=np.uint64)
    cs, cd, co = expected(name, phase, clip_ends, CLIP_OFF)
    clipped = clip_ends.astype(np.int64) - CLIP_OFF + 1 < m + k
    assert (clipped & (cd != NONE_DIST)).any() and (cd == NONE_DIST).any(), (name, cd.tolist())
    assert (cs[cd != NONE_DIST] >= CLIP_OFF).all()
    # (the inputs) occurrences below and at or above 2^32, by the find's own oracle on the period
    pos, _ = ref(0, 3 * U)
    residues = (pos[(pos >= U) & (pos < 2 * U)] - U - phase) % U  # away from the range's head, text positions congruent to these are ends
    assert len(residues) >= 1 and lo + 3 * U < BEYOND < lo + ln - 3 * U  # so each of them is met on both sides of 2^32
    text = Text.upload_tiled(tile, BEYOND_N, phase)
    try:
        assert len(text) == BEYOND_N
        for off in (BEYOND - 4096, BEYOND_N - 4096):
            assert np.array_equal(text.read(off, 4096), tiled_slice(tile, off, 4096, phase))
        ends, fdist = find_edit(P, text, k, off=lo, n=ln, cap=16 << 20)
        assert len(ends) > 0 and int(ends[0]) < BEYOND <= int(ends[-1])
        ws, wd, wo = expected(name, phase, ends, lo)
        assert np.array_equal(wd, fdist), name  # the oracle and the find agree on the distances before the align call is asked
        starts, dist, ops = align_edit(P, text, k, ends, off=lo, n=ln)
        assert np.array_equal(dist, wd), (name, first_difference(dist, wd, ends))
        assert np.array_equal(starts, ws), (name, first_difference(starts, ws, ends))
        assert np.array_equal(ops, wo), (name, first_difference((ops != wo).any(axis=1), np.zeros(len(ends), dtype=bool), ends))
        s2, d2, o2 = align_edit(P, text, k, ends, off=lo, n=ln, ops=False)
        assert o2 is None and np.array_equal(s2, ws) and np.array_equal(d2, wd), name
        # the range that begins beyond 2^32
        n2 = 4096
        for with_ops in (True, False):
            s, d, o = align_edit(P, text, k, clip_ends, off=CLIP_OFF, n=n2, ops=with_ops)
            assert np.array_equal(d, cd), (name, with_ops, first_difference(d, cd, clip_ends))
            assert np.array_equal(s, cs), (name, with_ops, first_difference(s, cs, clip_ends))
            assert (o is None) if not with_ops else np.array_equal(o, co), (name, with_ops)
    finally:
        text.free()


def first_difference(a, b, ends):
    at = int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])
    return at, int(ends[at]), int(a[at]), int(b[at])
