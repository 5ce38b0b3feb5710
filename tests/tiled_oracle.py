"""The exact answer of an approximate matcher over a TILED text (Text.upload_tiled: symbol i = unit[(phase + i) % U]) at any
size, from one of the suite's by-definition references run over three periods.  No test in here and no GPU use: the CPU
tests of tests/test_tiled_oracle.py hold expected_tiled to the direct reference on texts small enough to run it whole, the
GPU tests of tests/test_packed_at_size_gpu.py use it past 2^32 symbols.

Why three periods are enough.  An entry is a position p of the text and a distance; it is a START (the mis and sets calls: the
window [p, p + m) must lie in the range, span = m) or an END (the edit calls, span = 1).  Whether a start is reported depends
on the m symbols of its window alone.  Whether an end e is reported, and its distance, depends on at most m + k symbols
before it: a value <= k of Sellers' last row is the distance of a substring of at most m + k symbols that ends at e, and
values > k are not reported either way.  `warm` is that number of symbols (m, or m + k): from lo + warm on, an entry does
not see where the range began, so with U >= warm the entries of [lo + U, lo + 2U) repeat with period U up to the range's
end — and expected_tiled ASSERTS what it relies on, on the third period it computed."""
import numpy as np


def tiled_slice(unit, off, length, phase=0):
    """Symbols [off, off + length) of the tiled text, as Text.upload_tiled(unit, n, phase) builds it."""
    unit = np.asarray(unit, dtype=np.uint8)
    return unit[(int(phase) + int(off) + np.arange(int(length), dtype=np.int64)) % len(unit)]


def _computed(ref, U, lo, hi, warm, span):
    """The reference over the first 3 U symbols of [lo, hi) as (positions int64, distances uint8, symbols covered), after the
    checks: ascending positions inside the covered head, and the second and third period agree."""
    assert U >= warm >= span >= 1, "the unit (%d symbols) is shorter than what an entry depends on (%d)" % (U, warm)
    assert 0 <= lo <= hi
    L = min(3 * U, hi - lo)
    got = ref(lo, L)
    pos, dist = got if isinstance(got, tuple) else (got, None)
    pos = np.asarray(pos).astype(np.int64)
    dist = np.zeros(len(pos), dtype=np.uint8) if dist is None else np.asarray(dist).astype(np.uint8)
    assert len(pos) == len(dist) and (np.diff(pos) > 0).all()
    assert len(pos) == 0 or (pos[0] >= lo and pos[-1] + span <= lo + L)
    second = (pos >= lo + U) & (pos < lo + 2 * U) & (pos + U + span <= lo + L)
    third = pos >= lo + 2 * U
    assert np.array_equal(pos[second] + U, pos[third]) and np.array_equal(dist[second], dist[third]), \
        "the entries of the second and the third period differ: the answer is not periodic from lo + U on"
    return pos, dist, L


def expected_tiled(ref, U, lo, hi, warm, span=1):
    """(positions uint64, distances uint8), ascending, of the call over symbols [lo, hi) of a tiled text of period U.
    ref(off, length) is the by-definition reference on symbols [off, off + length) of that text ALONE (positions relative to
    symbol 0; a bare array of positions stands for distances 0).  span = m for calls that report starts, 1 for calls that
    report ends.  Entries below lo + 2U are taken as computed — the range's own head, where an edit call still sees the
    column before the range; later ones are the computed entries of [lo + U, lo + 2U) repeated with period U for as long as
    the entry's span ends inside the range."""
    pos, dist, L = _computed(ref, U, lo, hi, warm, span)
    if L == hi - lo:
        return pos.astype(np.uint64), dist
    head = pos < lo + 2 * U
    period = (pos >= lo + U) & head
    reps = np.arange(1, (hi - lo) // U + 1, dtype=np.int64) * U
    later = (reps[:, None] + pos[period][None, :]).ravel()
    keep = later + span <= hi
    dlater = np.broadcast_to(dist[period], (len(reps), int(period.sum()))).ravel()
    return np.concatenate([pos[head], later[keep]]).astype(np.uint64), np.concatenate([dist[head], dlater[keep]])


def expected_tiled_count(ref, U, lo, hi, warm, span=1):
    """len(expected_tiled(...)[0]) without building the list: each entry p of the period repeats for every j >= 1 with
    p + j U + span <= hi."""
    pos, dist, L = _computed(ref, U, lo, hi, warm, span)
    if L == hi - lo:
        return len(pos)
    head = pos < lo + 2 * U
    period = pos[(pos >= lo + U) & head]
    return int(head.sum()) + int(np.maximum((hi - span - period) // U, 0).sum())


def fold(pos, U, lo=0):
    """For every position its representative below lo + 2U: itself there, else the position of [lo + U, lo + 2U) that is a
    multiple of U below it.  What holds at the representative holds at the position, shifted by their difference."""
    pos = np.asarray(pos).astype(np.int64)
    return np.where(pos < lo + 2 * U, pos, lo + U + (pos - lo - U) % U)


def _other(vals, v, rng):
    rest = [x for x in vals if x != v]
    return rest[int(rng.integers(0, len(rest)))]


def edited(P, d, rng, vals, mixed, frozen=()):
    """P with d edits at distinct positions 1 <= j < len(P) - 1 outside `frozen`: substitutions, or with `mixed` the three
    kinds in turn (a substitution, a text symbol removed, a text symbol added that differs from the one before it).  The
    positions keep up to four symbols between them where the pattern has the room: an insertion next to a deletion is one
    substitution, and the copy would be nearer than d."""
    W = [int(x) for x in P]
    free = [j for j in range(1, len(W) - 1) if j not in frozen]
    free = free[::max(1, min(4, len(free) // max(d, 1)))]
    for t, j in enumerate(sorted(rng.choice(free, size=d, replace=False).tolist(), reverse=True)):
        if not mixed or t % 3 == 0:
            W[j] = _other(vals, W[j], rng)
        elif t % 3 == 1:
            del W[j]
        else:
            W.insert(j, _other(vals, W[j - 1], rng))
    return np.asarray(W, dtype=np.uint8)


def _nearest(P, W):
    """min over s of ed(P, W[s..]): how near the copy W is to P at its own end, whatever stands before it."""
    row = list(range(len(P) + 1))
    for c in W:
        diag, row[0] = row[0], 0
        for i in range(1, len(P) + 1):
            diag, row[i] = row[i], min(diag + (P[i - 1] != c), row[i] + 1, row[i - 1] + 1)
    return row[-1]


def make_unit(vals, P, k, U, seed, mixed=False, frozen=(), unit=None, planted=None, marks=True, ds=None):
    """(unit, planted): U uniform symbols over `vals` (or a copy of `unit`, to plant a further pattern into it) with copies of
    P that carry d = 0, 1, k // 2, k, k and k + 1 edits — substitutions only, or with `mixed` substitutions, insertions and
    deletions — spread over the unit, and with `marks` two more copies of d = min(k, 1) edits: one that wraps the unit's seam
    and one at unit offset (2^32 - len // 2) % U, which with phase 0 covers symbol 2^32 of the text.  `planted` lists
    (unit offset, length, d) of every copy, those of earlier calls included; no two copies touch.  `frozen`: pattern positions
    that are not edited (those of a set pattern that accept more than one symbol); `ds`: other numbers of edits than the six
    (a short unit has no room for eight copies of a long pattern)."""
    P = np.asarray(P, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    drawn = np.asarray(vals, dtype=np.uint8)[rng.integers(0, len(vals), U)]
    unit = drawn if unit is None else np.array(unit, dtype=np.uint8)
    assert len(unit) == U
    planted = list(planted or [])

    def free(a, n):
        return all((a - b) % U > ln and (b - a) % U > n for b, ln, _ in planted)

    def plant(a, W, d):
        a %= U
        for _ in range(U):
            if free(a, len(W)):
                break
            a = (a + 1) % U
        else:
            raise AssertionError("no room left in the unit")
        unit[(a + np.arange(len(W))) % U] = W
        planted.append((a, len(W), d))

    if marks:
        W = edited(P, min(k, 1), rng, vals, mixed, frozen)
        plant(U - len(W) // 2, W, min(k, 1))
        assert planted[-1][0] + len(W) > U  # it does wrap
        W = edited(P, min(k, 1), rng, vals, mixed, frozen)
        a = (2**32 - len(W) // 2) % U
        plant(a, W, min(k, 1))
        assert planted[-1][0] == a, "another copy already covers symbol 2^32"
    ds = (0, 1, k // 2, k, k, k + 1) if ds is None else ds
    for t, d in enumerate(ds):
        W = edited(P, d, rng, vals, mixed, frozen)
        while d > k and mixed and _nearest(P.tolist(), W.tolist()) <= k:  # on two values d edits are often fewer: draw again
            W = edited(P, d, rng, vals, mixed, frozen)
        plant(int(rng.integers(0, U // 64)) + (t + 1) * U // (len(ds) + 2), W, d)
    return unit, planted
