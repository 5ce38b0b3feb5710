"""The approximate matchers on packed texts AT SIZE: planes_sets_*, planes_mis_*, planes_sets_mis_*, planes_edit_*,
planes_editl_* and planes_edit_align on texts of 2^32 + 2^28 + 77 symbols — past one sweep of every grid (the launchers cap
the grid; the kernels walk the rest with `cw += stride`), past 2^32, and with a ragged last trip.  The text is a unit of
U = 2^18 + 13 symbols tiled on the device (Text.upload_tiled) and packed; what a call must return over any range follows from
the suite's by-definition references over three periods (tests/tiled_oracle.py, held to the direct reference by
tests/test_tiled_oracle.py).  U is odd: successive copies of the unit meet every phase of the 32-symbol dwords, the 128- and
512-symbol runs and the 8192-position spans.  Every comparison is exact equality.

What is in a unit and which cases run on it is decided here without a device (units(), CASE_NAMES): tests/test_tiled_oracle.py
imports both and asserts, from the references alone, that every case has between the planted copies and 512 entries per
period and at most 2^23 over the whole text."""
import functools
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (PackedText, Text, iupac_sets, palign_edit, pfind_edit, pfind_editl, pfind_mis, pfind_sets, pfind_sets_edit,  # noqa: E402
                       pfind_sets_mis, psearch_edit, psearch_editl, psearch_mis, psearch_sets, psearch_sets_edit, psearch_sets_mis)

import test_packed_mis_gpu as mis_gpu  # noqa: E402
import test_packed_sets_gpu as sets_gpu  # noqa: E402
import test_packed_sets_mis_gpu as sets_mis_gpu  # noqa: E402
from test_packed_align import NONE_DIST, NONE_START, align_many  # noqa: E402
from test_packed_edit import byte_accepts, edit_occurrences, set_accepts  # noqa: E402
from tiled_oracle import expected_tiled, expected_tiled_count, fold, make_unit, tiled_slice  # noqa: E402

ACGT = (65, 67, 71, 84)
BIN = (0, 255)
N = 2**32 + 2**28 + 77
U = 2**18 + 13
BEYOND = 2**32
# (off, length): one that straddles 2^32, unaligned, over more than one sweep of the planes and edit kernels; one wholly above
SUB_RANGES = [(2**32 - 2**27 - 45, 2**28 + 1001), (2**32 + 12345, 2**26 + 2**25 + 7)]
PER_PERIOD_MAX = 512
TOTAL_MAX = 2**23
MOTIF16 = "GANTCWGATNCAGTCA"                             # two N, one two-member position (W)
MOTIF40 = "TGCANGTCAGGCTWACGTACGNTCAGTCCGATAGCTAGGT"


def instance(motif):
    """A byte pattern the motif accepts, and the positions that accept more than one symbol."""
    wide = tuple(j for j, c in enumerate(motif) if c not in "ACGT")
    return np.frombuffer(motif.replace("N", "C").replace("W", "A").encode(), dtype=np.uint8).copy(), wide


def widened(P, vals):
    """Sets that accept the byte pattern P over `vals`: singletons, one position that accepts everything and one that accepts
    two values."""
    sets = (1 << np.searchsorted(np.asarray(vals, dtype=np.uint8), P)).astype(np.uint8)
    sets[len(P) // 4] = (1 << len(vals)) - 1
    sets[len(P) // 2] |= 1 if sets[len(P) // 2] != 1 else 2
    return sets


class Case:
    """One pattern of one family on one text: how the reference and the two calls are made for it."""

    def __init__(self, family, vals, kind, pat, k, planted, accepts=None):
        self.family, self.vals, self.kind, self.pat, self.k, self.planted, self.accepts = family, vals, kind, pat, k, planted, accepts
        self.m = len(pat)
        self.ends = family in ("edit", "sets_edit", "editl")
        self.warm = self.m + k if self.ends else self.m
        self.span = 1 if self.ends else self.m
        self.name = "%s-%s-m%d-k%d" % (family, "acgt" if vals == ACGT else "bin", self.m, k)

    def ref(self, off, length):
        """The by-definition reference of the family on symbols [off, off + length) of the tiled text alone."""
        S = tiled_slice(units()[self.vals, self.kind][0], off, length)
        if self.family == "sets":
            return sets_gpu.by_definition(self.pat, S, list(self.vals)).astype(np.int64) + off
        if self.family == "mis":
            pos, dist = mis_gpu.by_definition(self.pat, S, self.k)
        elif self.family == "sets_mis":
            pos, dist = sets_mis_gpu.by_definition(self.pat, S, self.vals, self.k)
        else:
            pos, dist = edit_occurrences(self.m, self.accepts, S, self.k)
        return pos.astype(np.int64) + off, dist

    def calls(self):
        """(what, count(pt, off, n), find(pt, off, n, cap)) for every form of the family's two calls."""
        p, k = self.pat, self.k
        if self.family == "sets":
            return [("", lambda pt, off, n: psearch_sets(p, pt, off=off, n=n), lambda pt, off, n, cap: pfind_sets(p, pt, off=off, n=n, cap=cap))]
        if self.family == "editl":
            return [("all_blocks=%s" % ab, lambda pt, off, n, ab=ab: psearch_editl(p, pt, k, off=off, n=n, all_blocks=ab),
                     lambda pt, off, n, cap, ab=ab: pfind_editl(p, pt, k, off=off, n=n, cap=cap, all_blocks=ab)) for ab in (False, True)]
        count, find = {"mis": (psearch_mis, pfind_mis), "sets_mis": (psearch_sets_mis, pfind_sets_mis), "edit": (psearch_edit, pfind_edit),
                       "sets_edit": (psearch_sets_edit, pfind_sets_edit)}[self.family]
        return [("", lambda pt, off, n: count(p, pt, k, off=off, n=n), lambda pt, off, n, cap: find(p, pt, k, off=off, n=n, cap=cap))]


@functools.lru_cache(maxsize=None)
def units():
    """{(vals, kind): (unit, cases)}: per value set one unit planted with substitutions only ('sub': the mis and sets calls) and
    one planted with substitutions, insertions and deletions ('mixed': the edit calls).  Every pattern has its own copies in
    the unit; the first pattern of a unit also owns the copy across the seam and the copy over symbol 2^32."""
    out = {}
    for vi, vals in enumerate((ACGT, BIN)):
        for ki, kind in enumerate(("sub", "mixed")):
            rng = np.random.default_rng(9000 + 10 * vi + ki)
            draw = lambda m: np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), m)]  # noqa: E731
            todo = []  # (pattern planted, k planted with, frozen, [(family, pat, k, accepts)])
            if kind == "sub":
                for m, k in ((20, 2), (33, 3), (64, 7)):
                    P = draw(m)
                    todo.append((P, k, (), [("mis", P, k, None)]))
                if vals == ACGT:
                    for motif in (MOTIF16, MOTIF40):
                        P, wide = instance(motif)
                        sets = iupac_sets(motif, vals)
                        todo.append((P, 2, wide, [("sets", sets, 0, None)] + ([("sets_mis", sets, 2, None)] if motif == MOTIF16 else [])))
            else:
                for m, k in ((20, 2), (33, 3), (64, 7)):
                    P = draw(m)
                    sets = widened(P, vals)
                    uses = [("edit", P, k, byte_accepts(P))]
                    if (vals, m) != (BIN, 20):  # widened sets of 20 positions on two values: 585 entries per period, over the cap
                        uses.append(("sets_edit", sets, k, set_accepts(sets, vals)))
                    if m == 64:                 # the long-pattern kernel on a length both kernels take
                        uses.append(("editl", P, k, byte_accepts(P)))
                    todo.append((P, k, (), uses))
                for m, k in ((100, 15), (256, 31)):
                    P = draw(m)
                    todo.append((P, k, (), [("editl", P, k, byte_accepts(P))]))
            unit, planted, cases = None, [], []
            for t, (P, k, frozen, uses) in enumerate(todo):
                before = len(planted)
                unit, planted = make_unit(vals, P, k, U, 9100 + 100 * vi + 10 * ki + t, mixed=kind == "mixed", frozen=frozen, unit=unit,
                                          planted=planted, marks=t == 0)
                cases += [Case(f, vals, kind, pat, kk, planted[before:], acc) for f, pat, kk, acc in uses]
            out[vals, kind] = (unit, cases)
    return out


CASE_NAMES = ["mis-acgt-m20-k2", "mis-acgt-m33-k3", "mis-acgt-m64-k7", "sets-acgt-m16-k0", "sets-acgt-m40-k0", "sets_mis-acgt-m16-k2",
              "mis-bin-m20-k2", "mis-bin-m33-k3", "mis-bin-m64-k7",
              "edit-acgt-m20-k2", "edit-acgt-m33-k3", "edit-acgt-m64-k7", "sets_edit-acgt-m20-k2", "sets_edit-acgt-m33-k3", "sets_edit-acgt-m64-k7",
              "editl-acgt-m64-k7", "editl-acgt-m100-k15", "editl-acgt-m256-k31",
              "edit-bin-m20-k2", "edit-bin-m33-k3", "edit-bin-m64-k7", "sets_edit-bin-m33-k3", "sets_edit-bin-m64-k7",
              "editl-bin-m64-k7", "editl-bin-m100-k15", "editl-bin-m256-k31"]
RANGED_NAMES = ["mis-acgt-m20-k2", "sets-acgt-m16-k0", "sets_mis-acgt-m16-k2", "edit-acgt-m20-k2", "editl-acgt-m64-k7", "mis-bin-m20-k2", "edit-bin-m20-k2"]


def case(name):
    found = [c for _, cases in units().values() for c in cases if c.name == name]
    assert len(found) == 1, name
    return found[0]


def expected(name, lo=0, hi=N):
    """The reference's answer for the case over [lo, hi), shared by the tests that follow each other on it; the arrays are not
    writable."""
    return _expected(name, lo, hi)


@functools.lru_cache(maxsize=4)
def _expected(name, lo, hi):
    c = case(name)
    pos, dist = expected_tiled(c.ref, U, lo, hi, c.warm, c.span)
    pos.setflags(write=False)
    dist.setflags(write=False)
    return pos, dist


def trips(cus, n=N):
    """Trips of the grid-stride loop that n symbols need on `cus` compute units, per kernel family: a sweep is the capped grid
    (8 workgroups per CU; 7 for the two-plane mismatch counter with three bits) times 256 lanes times what a lane owns."""
    sweep = {"sets, mis, sets_mis": cus * 8 * 256 * 2 * 128, "mis on two planes, k >= 4": cus * 7 * 256 * 2 * 128, "edit": cus * 8 * 256 * 128,
             "editl": cus * 8 * 256 * 512}
    return {f: -(-n // s) for f, s in sweep.items()}


# ---- the texts -----------------------------------------------------------------------------------------------------------

_texts = {}


def compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, read in a child process: torch brings a HIP runtime of its
    own, which finds no device in a process where libsmartgpu.so's runtime already holds it."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


@pytest.fixture(scope="module", autouse=True)
def texts():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()
    cus = compute_units()
    # more than two sweeps of the widest grid (planes_editl_*): on a larger part this fails instead of running one trip
    assert N >= 2 * cus * 8 * 256 * 512 + 1, (N, cus)
    print("compute units %d, trips over %d symbols: %s" % (cus, N, trips(cus)))
    yield _texts
    while _texts:
        _texts.popitem()[1].free()


def packed(vals, kind):
    """The packed tiled text of a unit, made at its first use; the byte text is freed right after packing."""
    if (vals, kind) not in _texts:
        unit, cases = units()[vals, kind]
        text = Text.upload_tiled(unit, N)
        try:
            pt = PackedText.pack(text)
        finally:
            text.free()
        _texts[vals, kind] = pt
        assert len(pt) == N and pt.symbols() == list(vals) and pt.planes == (2 if len(vals) > 2 else 1)
        for off in (0, BEYOND - 4096, N - 4096):
            assert np.array_equal(pt.read(off, 4096), tiled_slice(unit, off, 4096)), (vals, kind, off)
        # (the inputs, by the reference alone) entries on both sides of 2^32 and a window that contains symbol 2^32
        owner = cases[0]
        pos = expected(owner.name)[0].astype(np.int64)
        assert pos[0] < BEYOND < pos[-1]
        if owner.ends:  # a match that ends at e has at least m - k symbols
            assert ((pos >= BEYOND) & (pos < BEYOND + owner.m - owner.k)).any()
        else:
            assert ((pos <= BEYOND) & (pos + owner.m > BEYOND)).any()
    return _texts[vals, kind]


def check(name, lo, hi):
    c = case(name)
    pt = packed(c.vals, c.kind)
    wpos, wdist = expected(name, lo, hi)
    assert len(wpos) > 0
    for what, count, find in c.calls():
        got = count(pt, lo, hi - lo)[0]
        assert got == len(wpos), (name, what, lo, hi, got, len(wpos))
        res = find(pt, lo, hi - lo, len(wpos))
        pos, cnt = res[0], res[-1]
        assert cnt == len(wpos) and pos is not None and pos.dtype == np.uint64 and len(pos) == cnt, (name, what, lo, hi, cnt, len(wpos))
        assert np.array_equal(pos, wpos), (name, what, lo, hi, first_difference(pos, wpos))
        if len(res) == 3:
            assert res[1].dtype == np.uint8 and np.array_equal(res[1], wdist), (name, what, lo, hi, first_difference(res[1], wdist))


def first_difference(a, b):
    at = int(np.flatnonzero(a != b)[0])
    return at, int(a[at]), int(b[at])


# ---- the cases -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASE_NAMES)
def test_whole_text(name):
    """Count call and find call (for planes_editl_* with the cut-off and with all blocks) over all 2^32 + 2^28 + 77 symbols."""
    check(name, 0, N)
    pos = expected(name)[0]
    assert int(pos[0]) < BEYOND < int(pos[-1])


@pytest.mark.parametrize("off,ln", SUB_RANGES)
@pytest.mark.parametrize("name", RANGED_NAMES)
def test_sub_ranges(name, off, ln):
    """A range's answer is the programme on the range alone: the reference runs on the range's own head."""
    check(name, off, off + ln)


@pytest.mark.parametrize("ops", [True, False])
@pytest.mark.parametrize("name", ["edit-bin-m20-k2", "edit-acgt-m64-k7"])
def test_alignments_at_size(name, ops):
    """planes_edit_align (one dword and two) on 2^20 ends of pfind_edit's result: every end in the copies of the unit around
    symbol 2^32, every end of the last copy and the ragged tail, a seeded sample of the rest — where the find has fewer than
    2^20 ends, all of them and some twice — and a few ends that are no occurrence, shuffled.  The starts, distances and
    operations at an end are those at its representative in the first two periods (align_many on that slice), the starts
    shifted by the difference."""
    c = case(name)
    pt = packed(c.vals, c.kind)
    wpos, wdist = expected(name)
    ends, dist, cnt = pfind_edit(c.pat, pt, c.k, cap=len(wpos))
    assert cnt == len(wpos) and np.array_equal(ends, wpos) and np.array_equal(dist, wdist)
    e = ends.astype(np.int64)
    j0 = BEYOND // U
    must = ((e >= (j0 - 1) * U) & (e < (j0 + 2) * U)) | (e >= (N // U - 1) * U)
    rng = np.random.default_rng(4242)
    misses = np.concatenate([rng.integers(0, N, 14), [0, BEYOND - 1, BEYOND, N - 1]])
    misses = misses[~np.isin(misses, e)]
    assert len(misses) >= 8 and (misses >= BEYOND).any() and (misses < BEYOND).any()
    rest = np.flatnonzero(~must)
    total = 2**20
    room = total - int(must.sum()) - len(misses)
    assert must.sum() > 0 and room > 0
    sample = rng.choice(rest, size=room, replace=False) if len(rest) >= room else np.concatenate([rest, rng.choice(len(e), size=room - len(rest))])
    chosen = np.concatenate([e[must], e[sample], misses])
    rng.shuffle(chosen)
    assert len(chosen) == total and (chosen > BEYOND).any() and (chosen < BEYOND).any()
    rep = fold(chosen, U)
    uniq, inv = np.unique(rep, return_inverse=True)
    ustarts, udist, uops = align_many(c.m, c.accepts, tiled_slice(units()[c.vals, c.kind][0], 0, 2 * U), uniq, c.k)
    hit = udist[inv] != NONE_DIST
    wstarts = np.where(hit, ustarts[inv] + (chosen - rep).astype(np.uint64), NONE_START)
    assert hit.sum() == total - len(misses)
    starts, adist, aops = palign_edit(c.pat, pt, c.k, chosen, ops=ops)
    assert starts.dtype == np.uint64 and adist.dtype == np.uint8
    assert np.array_equal(starts, wstarts), first_difference(starts, wstarts)
    assert np.array_equal(adist, udist[inv])
    if ops:
        assert aops.dtype == np.uint64 and aops.shape == (total, 3) and np.array_equal(aops, uops[inv])
    else:
        assert aops is None


@pytest.mark.parametrize("family", ["mis", "edit"])
def test_counts_beyond_2_to_the_32(family):
    """An 8-symbol pattern at k = 7 on the two-value text: nearly every position is an occurrence, the count does not fit 32
    bits.  The expected number comes from the count-only form of the oracle; a find with no room returns it too."""
    unit = units()[BIN, "sub"][0]
    pt = packed(BIN, "sub")
    P8 = np.array([0, 255, 255, 0, 255, 0, 0, 0], dtype=np.uint8)
    if family == "mis":
        def ref(off, length):
            pos, dist = mis_gpu.by_definition(P8, tiled_slice(unit, off, length), 7)
            return pos.astype(np.int64) + off, dist
        want = expected_tiled_count(ref, U, 0, N, 8, 8)
        got, none = psearch_mis(P8, pt, 7)[0], pfind_mis(P8, pt, 7, cap=0)
    else:
        def ref(off, length):
            pos, dist = edit_occurrences(8, byte_accepts(P8), tiled_slice(unit, off, length), 7)
            return pos.astype(np.int64) + off, dist
        want = expected_tiled_count(ref, U, 0, N, 15, 1)
        got, none = psearch_edit(P8, pt, 7)[0], pfind_edit(P8, pt, 7, cap=0)
    assert want > 2**32
    assert got == want, (family, got, want)
    assert none == (None, None, want), (family, none[2], want)


def test_a_cap_one_short_returns_the_count_alone():
    name = "edit-acgt-m20-k2"
    c = case(name)
    count = len(expected(name)[0])
    assert pfind_edit(c.pat, packed(c.vals, c.kind), c.k, cap=count - 1) == (None, None, count)
