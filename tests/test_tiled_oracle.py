"""tests/tiled_oracle.py without a GPU.  On a tiled text small enough for the direct reference (U = 1013, n = 10 U + 77,
materialised with np.resize) expected_tiled equals the reference over the whole range, for every family and over ranges
that start and end anywhere; the count-only form agrees with the list; a unit shorter than what an entry depends on is
refused.  And the INPUTS of tests/test_packed_at_size_gpu.py, at its real U and from the references alone: every case has
at least the planted copies and at most 512 entries per period, at most 2^23 over the whole text, the copies planted with
up to k edits are entries and those with k + 1 are not."""
import numpy as np
import pytest

from smart_amd import iupac_sets

import test_packed_at_size_gpu as at_size
import test_packed_mis_gpu as mis_gpu
import test_packed_sets_gpu as sets_gpu
import test_packed_sets_mis_gpu as sets_mis_gpu
from test_packed_edit import byte_accepts, edit_occurrences
from tiled_oracle import expected_tiled, expected_tiled_count, make_unit, tiled_slice

ACGT = (65, 67, 71, 84)
U = 1000 + 13
N = 10 * U + 77
RANGES = [(0, N), (1, N - 1), (U + 5, 6 * U + 3), (7, U + 507)]
MOTIF = "GANTCWGATNCAGTCA"


def small(family, m, k):
    """(unit, the family's reference on a slice S with positions relative to S, warm, span) for one pattern planted in U symbols."""
    rng = np.random.default_rng(100 * m + k)
    mixed = family == "edit"
    frozen = ()
    if family in ("sets", "sets_mis"):
        P, frozen = at_size.instance(MOTIF)
        sets = iupac_sets(MOTIF, ACGT)
    else:
        P = np.asarray(ACGT, dtype=np.uint8)[rng.integers(0, 4, m)]
    ds = None if m <= 64 else (0, k, k + 1)
    unit, planted = make_unit(ACGT, P, max(k, 2) if family == "sets" else k, U, 7 + m + k, mixed=mixed, frozen=frozen, ds=ds)
    assert len(planted) == (8 if ds is None else 5) and len(unit) == U
    if family == "mis":
        on = lambda S: mis_gpu.by_definition(P, S, k)  # noqa: E731
    elif family == "sets":
        on = lambda S: (sets_gpu.by_definition(sets, S, list(ACGT)), None)  # noqa: E731
    elif family == "sets_mis":
        on = lambda S: sets_mis_gpu.by_definition(sets, S, ACGT, k)  # noqa: E731
    else:
        on = lambda S: edit_occurrences(m, byte_accepts(P), S, k)  # noqa: E731
    return unit, on, (m + k if mixed else m), (1 if mixed else m)


SMALL = [("mis", 20, 2), ("sets", 16, 0), ("sets_mis", 16, 2), ("edit", 20, 2), ("edit", 64, 7), ("edit", 100, 15)]


@pytest.mark.parametrize("family,m,k", SMALL)
def test_expected_tiled_equals_the_reference_over_the_whole_range(family, m, k):
    unit, on, warm, span = small(family, m, k)
    T = np.resize(unit, N)
    assert np.array_equal(T[U - 3:3 * U + 2], tiled_slice(unit, U - 3, 2 * U + 5))

    def ref(off, length):
        pos, dist = on(tiled_slice(unit, off, length))
        return (pos.astype(np.int64) + off, dist) if dist is not None else pos.astype(np.int64) + off

    for lo, hi in RANGES:
        wpos, wdist = on(T[lo:hi])
        wpos = wpos + np.uint64(lo)
        wdist = np.zeros(len(wpos), dtype=np.uint8) if wdist is None else wdist
        pos, dist = expected_tiled(ref, U, lo, hi, warm, span)
        assert pos.dtype == np.uint64 and dist.dtype == np.uint8
        assert np.array_equal(pos, wpos) and np.array_equal(dist, wdist), (family, m, k, lo, hi)
        assert expected_tiled_count(ref, U, lo, hi, warm, span) == len(wpos)
        assert len(wpos) >= 2 and (hi - lo < 3 * U or int(wpos[-1]) >= lo + 3 * U)  # entries, and some from the repeated part


def test_a_unit_shorter_than_what_an_entry_depends_on_is_refused():
    def ref(off, length):
        raise RuntimeError("refused before the reference runs")
    for form in (expected_tiled, expected_tiled_count):
        with pytest.raises(AssertionError, match="shorter"):
            form(ref, 21, 0, 500, 22)
        with pytest.raises(RuntimeError):
            form(ref, 22, 0, 500, 22)


def test_a_reference_that_is_not_periodic_is_refused():
    """The check expected_tiled makes on the third period: a reference with one entry that does not repeat."""
    ref = lambda off, length: np.array([x for x in (off + 5, off + U + 5, off + 2 * U + 6) if x < off + length], dtype=np.int64)  # noqa: E731
    with pytest.raises(AssertionError, match="periodic"):
        expected_tiled(ref, U, 0, N, 1)


# ---- the inputs of the tests at size ---------------------------------------------------------------------------------------

def test_the_case_lists_name_what_the_units_hold():
    held = sorted(c.name for _, cases in at_size.units().values() for c in cases)
    assert held == sorted(at_size.CASE_NAMES) and set(at_size.RANGED_NAMES) <= set(held)
    for (vals, kind), (unit, cases) in at_size.units().items():
        assert len(unit) == at_size.U and sorted(set(unit.tolist())) == sorted(vals)
        spots = sorted({(a, ln) for c in cases for a, ln, _ in c.planted})
        assert all(a + ln < b for (a, ln), (b, lb) in zip(spots, spots[1:]))                          # no two copies touch
        assert any((a + ln > at_size.U) for a, ln in spots)                                           # one wraps the seam
        assert any(a <= 2**32 % at_size.U < a + ln for a, ln in spots)                                # one covers symbol 2^32
    assert at_size.U % 2 == 1 and at_size.N > 2**32 + 2**28  # more than one planes_editl sweep of 256 CUs beyond 2^32


@pytest.mark.parametrize("name", at_size.CASE_NAMES)
def test_inputs_at_size(name):
    c = at_size.case(name)
    BU = at_size.U
    pos, dist = expected_tiled(c.ref, BU, 0, 3 * BU, c.warm, c.span)
    pos = pos.astype(np.int64)
    period = (pos >= BU) & (pos < 2 * BU)
    found = dict(zip((pos[period] - BU).tolist(), dist[period].tolist()))
    within = [(a, ln, d) for a, ln, d in c.planted if d <= c.k]
    total = expected_tiled_count(c.ref, BU, 0, at_size.N, c.warm, c.span)
    print("%s: %d entries per period, %d over the whole text, %d of %d planted copies within k" % (name, len(found), total, len(within), len(c.planted)))
    assert 1 <= len(within) <= len(found) <= at_size.PER_PERIOD_MAX, (name, len(found))
    assert total <= at_size.TOTAL_MAX, (name, total)
    for a, ln, d in c.planted:
        at = (a + ln - 1) % BU if c.ends else a
        if d <= c.k:
            assert at in found and (found[at] <= d if c.ends else found[at] == d), (name, a, ln, d, found.get(at))
        elif not c.ends or c.family != "sets_edit":
            assert at not in found, (name, a, ln, d, found[at])  # k + 1 edits: not reported
    for lo, ln in at_size.SUB_RANGES if name in at_size.RANGED_NAMES else []:
        assert 0 < expected_tiled_count(c.ref, BU, lo, lo + ln, c.warm, c.span) <= at_size.TOTAL_MAX
