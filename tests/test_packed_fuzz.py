"""tests/packed_fuzz.py without a GPU: draw is a pure function of (family, index, seed); every case it draws is inside the
legal arguments of its calls and inside the bound on the reference's work; the committed seed and counts meet the strata
tests/test_packed_fuzz_gpu.py closes with, by the generator and the references alone; and on small cases of the same
generator (at most 60 symbols, patterns of at most 12) the references the fuzz trusts equal the cell-by-cell definitions:
plain_dp for the edit families, a triple loop for the Hamming families, align_one for the alignments."""
import functools

import numpy as np
import pytest

from smart_amd import engine, iupac_sets

import packed_fuzz as pf
from test_packed_align import NONE_DIST, NONE_START, align_many, align_one, pack_ops
from test_packed_edit import plain_dp


@pytest.fixture(scope="module", autouse=True)
def built():
    engine.build()  # iupac_sets is the library's


@functools.lru_cache(maxsize=None)
def committed(family):
    cases = [pf.draw(family, index) for index in range(pf.CASES[family])]
    for c in cases:
        c.T.setflags(write=False)
        c.pat.setflags(write=False)
    return cases


def same(a, b):
    return (a.S == b.S and a.vals == b.vals and np.array_equal(a.T, b.T) and np.array_equal(a.pat, b.pat) and a.sets == b.sets and a.k == b.k
            and a.ranges == b.ranges and a.all_blocks == b.all_blocks and a.shape() == b.shape() and a.motif == b.motif
            and (a.twin is None) == (b.twin is None) and (a.twin is None or np.array_equal(a.twin, b.twin)))


@pytest.mark.parametrize("family", pf.FAMILIES)
def test_draw_is_a_pure_function_of_its_arguments(family):
    first = [pf.draw(family, i) for i in (0, 1, 7, 30)]
    again = [pf.draw(family, i) for i in (30, 7, 1, 0)][::-1]  # in another order, other cases drawn in between
    assert all(same(a, b) for a, b in zip(first, again))
    assert not same(pf.draw(family, 7), pf.draw(family, 7, seed=pf.SEED + 1))
    assert not same(pf.draw(family, 7), pf.draw(family, 8))
    lists = [pf.end_lists(first[1], 0, np.arange(0, len(first[1].T), 3)) for _ in range(2)]
    assert all(np.array_equal(a, b) for a, b in zip(*lists))


@pytest.mark.parametrize("family", pf.FAMILIES)
def test_every_case_is_inside_the_calls_legal_arguments(family):
    for c in committed(family):
        say = c.shape()
        n = len(c.T)
        assert c.family == family and 1 <= n <= pf.MAX_N and c.T.dtype == np.uint8, say
        assert c.vals == tuple(np.unique(c.T).tolist()) and 1 <= len(c.vals) <= 4 and set(c.vals) <= set(c.S), say
        assert c.pat.dtype == np.uint8 and 1 <= c.m <= pf.MAX_M[family] and 0 <= c.k <= pf.MAX_K[family], say
        assert c.sets == (family in ("sets", "sets_mis")) or family in ("edit", "editl", "align"), say
        if c.sets:  # never a bit at or above the number of values the text holds
            assert int(c.pat.max()) < 1 << len(c.vals), say
        if c.twin is not None:
            assert c.sets and np.array_equal(pf.singleton_sets(c.twin, c.vals), c.pat), say
        if c.motif is not None:
            assert np.array_equal(iupac_sets(c.motif, c.vals), c.pat), say
        assert c.ranges[0] == (0, n) and len(c.ranges) == (2 if n >= 2 else 1), say
        for off, ln in c.ranges[1:]:
            assert off % 32 != 0 and ln >= 1 and off + ln <= n, say
        # the bound on the reference's work
        if family not in pf.HAMMING or c.text_kind != "uniform" or len(c.S) == 1:
            assert n * c.m <= max(pf.WORK, n), say
        if family == "align":
            for r, (off, ln) in enumerate(c.ranges):
                for ends in pf.end_lists(c, r, pf.reference(c, off, ln)[0]):
                    assert ends.dtype == np.uint64 and len(ends) <= pf.ALIGN_ENDS and (len(ends) == 0 or (off <= int(ends.min()) and int(ends.max()) < off + ln)), say


@pytest.mark.parametrize("family", pf.FAMILIES)
def test_the_committed_run_meets_its_strata(family):
    cases = committed(family)
    shapes = [pf.answer_shape(c) for c in cases]
    assert pf.missing_strata(family, cases, shapes) == []
    # the generator can fail the condition: a run of one case does
    assert pf.missing_strata(family, cases[:1], shapes[:1]) != []
    if family in ("sets", "sets_mis", "edit", "editl", "align"):
        assert any(c.motif is not None for c in cases) and any(c.twin is not None for c in cases)
    assert any(0 in c.vals for c in cases) and any(255 in c.vals for c in cases) and any(c.vals == pf.ACGT for c in cases)
    foreign = [c for c in cases if not c.sets and not set(c.pat.tolist()) <= set(c.S)]
    empty = [c for c in cases if c.sets and (c.pat == 0).any()]
    full = [c for c in cases if c.sets and (c.pat == (1 << len(c.vals)) - 1).any()]
    assert (foreign or family in ("sets", "sets_mis")) and (empty and full or family == "mis")


# ---- the references against the cell-by-cell definitions, on the fuzz's own kinds of input ----------------------------------

def hamming_by_loops(accepts_symbol, m, T, k, off, n):
    """The definition of the Hamming families as a triple loop: for every start, for every pattern position, a comparison."""
    pos, dist = [], []
    for s in range(off, off + n - m + 1):
        d = 0
        for j in range(m):
            d += 0 if accepts_symbol(j, int(T[s + j])) else 1
        if d <= k:
            pos.append(s)
            dist.append(d)
    return pos, dist


def symbol_test(c):
    """accepts(j, symbol) of a case, from its pattern alone."""
    if not c.sets:
        return lambda j, s: int(c.pat[j]) == s
    return lambda j, s: s in c.vals and bool(int(c.pat[j]) >> c.vals.index(s) & 1)


@pytest.mark.parametrize("family", pf.FAMILIES)
def test_the_references_equal_the_definitions_on_small_drawn_cases(family):
    answers = 0
    for index in range(60):
        c = pf.draw(family, index, small=True)
        assert len(c.T) <= 60 and c.m <= 12
        acc = symbol_test(c)
        for r, (off, n) in enumerate(c.ranges):
            pos, dist = pf.reference(c, off, n)
            assert pos.dtype == np.uint64 and dist.dtype == np.uint8
            if family in pf.HAMMING:
                wpos, wdist = hamming_by_loops(acc, c.m, c.T, c.k, off, n)
            else:
                D = plain_dp(acc, c.m, c.T[off:off + n])
                wpos = [off + e for e, d in enumerate(D) if d <= c.k]
                wdist = [d for d in D if d <= c.k]
            assert pos.tolist() == wpos and dist.tolist() == wdist, c.shape()
            answers += len(wpos)
            if family == "align":
                ends = np.concatenate(pf.end_lists(c, r, pos))
                starts, d, words = align_many(c.m, c.accepts(), c.T, ends, c.k, off)
                for x, e in enumerate(ends.tolist()):
                    one = align_one(c.m, c.accepts(), c.T, e, c.k, off)
                    if one is None:
                        assert starts[x] == NONE_START and d[x] == NONE_DIST and not words[x].any(), c.shape()
                    else:
                        assert (int(starts[x]), int(d[x]), words[x].tolist()) == (one[0], one[1], pack_ops(one[2])), c.shape()
    assert answers > 0
