"""The generator and the checks of the differential fuzz for the approximate matchers on packed texts.  No test in here:
tests/test_packed_fuzz.py holds the generator to its promises without a GPU, tests/test_packed_fuzz_gpu.py runs the committed
seed and counts on the GPU, tools/packed_fuzz_gpu.py is the open-ended form.

draw(family, index, seed) is a pure function of its arguments — one generator seeded with (seed, family, index), no state
between cases — so a failure is reproduced anywhere from the two numbers alone.  Six families: `sets` (psearch_sets /
pfind_sets), `mis`, `sets_mis`, `edit` and `editl` (each draws the byte form or the sets form of its calls), and `align`
(palign_edit / palign_sets_edit on the ends of the edit find).

What a case holds, in the order it is drawn:
  the value set    1 .. 4 distinct bytes, 0 and 255 likely, ACGT in every fourth case;
  the text length  tiny (1 .. 100), around a lane's or a wave's run of the family's kernels +- 40, or up to two workgroups'
                   runs and a ragged tail, never more than 2^18 + 77 symbols: one grid sweep (GEOMETRY);
  the base text    uniform, skewed (one value at 90 %), a unit of 1 .. 9 symbols with sparse point mutations, geometric runs,
                   one value only, or SEGMENTS of these kinds with lengths around the lane run and the wave run;
  m and k          every k the call takes, m with the edges of the kernels' column widths; k >= m happens;
  the pattern      a window of the text with 0, k - 1, k or k + 1 edits (substitutions for the Hamming families, the three
                   kinds for the edit families), periodic, bordered (u v u) or random; then u foreign bytes, u <= k or k + 1;
                   for editl also GAPPED (see GAPPED below): a run of positions that accept nothing inside the pattern;
                   for the sets forms: singletons (the byte call must agree), IUPAC-like or random sets with empty and full
                   ones — as subsets of the value set, turned into bits over the values the finished text holds, so no
                   set ever names a code the text does not hold;
  the ranges       the whole text and one (off, n) with off % 32 != 0 that mostly ends mid-dword; for the edit families
                   sometimes n < m <= n + k or n + k < m;
  the field        in a segmented text one segment is a FIELD of near-copies — an instance of the pattern repeated with 0 ..
                   k + 1 edits per copy — next to a uniform segment, both shorter than a wave's run: half of a wave's lanes sit in
                   near-copies, the other half in noise;
  the copies       instances with d <= k edits planted at random places, at each range's first symbol and up to its last.
A one-value text stays one value: nothing is planted into it.

THE BOUND ON THE REFERENCE'S WORK.  No case is ever skipped; instead the pattern is shortened until n * m <= WORK = 2^25
wherever the reference costs n * m: always for the edit families (edit_row makes m passes over the range: 0.33 s at 2^18 x
256, so at most 0.17 s here), and for the Hamming families on every text but a uniform one over two or more values (by_definition
keeps every candidate of a dense text: 2.0 s at 2^18 x 4200, at most 0.06 s here).  align_many holds (m + 1) (m + k + 1) cells
per end: every list of ends has at most ALIGN_ENDS = 256 entries."""
import numpy as np

import test_packed_mis_gpu as mis_gpu
import test_packed_sets_gpu as sets_gpu
import test_packed_sets_mis_gpu as sets_mis_gpu
from test_packed_align import NONE_DIST, NONE_START, align_many, replay, unpack_ops
from test_packed_edit import byte_accepts, edit_row, set_accepts

SEED = 20261019
FAMILIES = ("sets", "mis", "sets_mis", "edit", "editl", "align")
# cases of the committed run per family (tests/test_packed_fuzz_gpu.py says what they cost); the floor is missing_strata() == []
CASES = {"sets": 256, "mis": 256, "sets_mis": 256, "edit": 256, "editl": 128, "align": 96}
HAMMING = ("sets", "mis", "sets_mis")
ACGT = (65, 67, 71, 84)
# symbols a lane, a wave and a workgroup own in one trip: 128 start positions per lane and kFindSpan = 8192 per wave for the
# plane kernels (a workgroup of 256 lanes takes two spans per wave), kEditRun = 128 and kEditlRun = 512 end positions per lane
GEOMETRY = {"sets": (128, 8192, 65536), "mis": (128, 8192, 65536), "sets_mis": (128, 8192, 65536),
            "edit": (128, 8192, 32768), "align": (128, 8192, 32768), "editl": (512, 32768, 131072)}
MAX_N = 2**18 + 77
MAX_M = {"sets": 4200, "mis": 4200, "sets_mis": 4200, "edit": 64, "align": 64, "editl": 256}
MAX_K = {"sets": 0, "mis": 7, "sets_mis": 7, "edit": 7, "align": 7, "editl": 31}
WORK = 2**25
ALIGN_ENDS = 256
TEXT_KINDS = ("uniform", "skewed", "periodic", "runs", "one_value", "segments")
PATTERN_KINDS = ("window", "periodic", "bordered", "random")
# editl only: a prefix, a run of k - 3 .. k positions that accept nothing, a suffix, at k = 29 .. 31, and the text holds forty
# times prefix and suffix with 0 .. 36 symbols between them.  The run's block is all +1 with no match bit, so the carry of the addition in
# block_step passes THROUGH a whole dword into the next block — the one input on which the term "s < s1" of the carry matters
# for a value <= k (profiles/packed/RESULTS.md, "Differential fuzz", mutant L)
GAPPED = "gapped"
SET_KINDS = ("singleton", "iupac", "random")
IUPAC = {1: "A", 2: "C", 4: "G", 8: "T", 5: "R", 10: "Y", 6: "S", 9: "W", 12: "K", 3: "M", 14: "B", 13: "D", 11: "H", 7: "V", 15: "N"}


class Case:
    """One drawn case.  family, index, seed; S the value set drawn, vals the values the finished text holds (what
    PackedText.symbols() returns); T the text; pat what the call takes (bytes, or sets over vals) and sets whether it is sets;
    twin a byte pattern that must give the same answers as a singleton-set pattern (or None); motif the IUPAC letters of an
    IUPAC-like pattern over ACGT (or None); k; all_blocks (editl: the form held to the reference; the other is held to it by
    the identity); ranges [(off, n)]; and what was drawn, for the strata: text_kind, stratum, pattern_kind, set_kind, field."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.m = len(self.pat)

    def accepts(self, pat=None, sets=None):
        pat = self.pat if pat is None else pat
        return set_accepts(pat, self.vals) if (self.sets if sets is None else sets) else byte_accepts(pat)

    def shape(self):
        return "(%s, %d) seed %d: %d values %s, n %d (%s, %s%s), m %d, k %d, %s pattern (%s%s), ranges %s" % (
            self.family, self.index, self.seed, len(self.vals), list(self.vals), len(self.T), self.stratum, self.text_kind,
            " with a field" if self.field else "", self.m, self.k, "sets" if self.sets else "byte", self.pattern_kind,
            ", " + self.set_kind if self.sets else "", self.ranges)


# ---- the pieces --------------------------------------------------------------------------------------------------------------

def _values(rng, index):
    if index % 4 == 0:
        return ACGT
    nv = int(rng.choice([1, 2, 3, 4], p=[0.1, 0.35, 0.2, 0.35]))
    pool = [v for v in (0, 255) if rng.random() < 0.4]
    rng.shuffle(pool)
    pool = pool[:nv]
    while len(pool) < nv:
        v = int(rng.integers(0, 256))
        if v not in pool:
            pool.append(v)
    return tuple(sorted(pool))


def _length(rng, family):
    lane, wave, wg = GEOMETRY[family]
    r = rng.random()
    if r < 0.3:
        return "tiny", int(rng.integers(1, 101))
    if r < 0.75:
        return "around", max(1, int(rng.choice([lane, wave])) + int(rng.integers(-40, 41)))
    return "large", min(MAX_N, int(rng.integers(wave + 41, 2 * wg + 1)) + int(rng.integers(1, 78)))


def _base(rng, S, n, kind):
    """n symbols over S of one of the plain kinds."""
    S = np.asarray(S, dtype=np.uint8)
    if kind == "one_value" or len(S) == 1:
        return np.full(n, S[int(rng.integers(0, len(S)))], dtype=np.uint8)
    if kind == "uniform":
        return S[rng.integers(0, len(S), n)]
    if kind == "skewed":
        p = np.full(len(S), 0.1 / (len(S) - 1))
        p[int(rng.integers(0, len(S)))] = 0.9
        return S[rng.choice(len(S), size=n, p=p)]
    if kind == "periodic":
        T = np.resize(S[rng.integers(0, len(S), int(rng.integers(1, 10)))], n).copy()
        hit = np.flatnonzero(rng.random(n) < 1 / 150)
        T[hit] = S[rng.integers(0, len(S), len(hit))]
        return T
    assert kind == "runs", kind
    lengths = rng.geometric(1 / float(rng.choice([3, 12, 60])), size=n)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), n)) + 1]
    codes = np.cumsum(rng.integers(1, len(S), len(lengths))) % len(S)  # every run differs from the one before it
    return S[np.repeat(codes, lengths)[:n]]


def _edits(W, d, rng, S, mixed):
    """W with d edits at random places: substitutions, or with `mixed` substitutions, symbols removed and symbols added.  (On
    one value a substitution is no edit: then a symbol is removed or added where that is allowed.)"""
    W = [int(x) for x in W]
    for _ in range(d):
        j = int(rng.integers(0, len(W)))
        op = int(rng.integers(0, 3)) if mixed else 0
        if op == 0 and len(S) == 1:
            op = 1 if mixed else 3
        if op == 0:
            rest = [v for v in S if v != W[j]]
            W[j] = int(rest[int(rng.integers(0, len(rest)))])
        elif op == 1 and len(W) > 1:
            del W[j]
        elif op in (1, 2):
            W.insert(j, int(S[int(rng.integers(0, len(S)))]))
    return np.asarray(W, dtype=np.uint8)


def _fit(P, m, rng, S):
    """P cut or filled up with random symbols to m symbols."""
    if len(P) >= m:
        return np.asarray(P[:m], dtype=np.uint8)
    return np.concatenate([P, np.asarray(S, dtype=np.uint8)[rng.integers(0, len(S), m - len(P))]]).astype(np.uint8)


def _m_and_k(rng, family, index, n, dense):
    if family == "editl":
        bucket = int(rng.integers(0, 4))
        k = 31 if bucket == 3 else int(rng.integers(*[(0, 8), (8, 16), (16, 32)][bucket]))
        edges = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 255, 256]
        lo, hi = [(1, 64), (65, 128), (129, 256)][int(rng.integers(0, 3))]
        m = int(rng.choice(edges)) if rng.random() < 0.4 else int(rng.integers(lo, hi + 1))
    elif family in HAMMING:
        k = 0 if family == "sets" else index % 8
        r = rng.random()
        m = (int(rng.choice([1, 2, 3, 31, 32, 33, 63, 64, 65])) if r < 0.3 else int(rng.integers(1, 131)) if r < 0.8
             else int(np.exp(rng.uniform(np.log(131), np.log(4201)))))
    else:
        k = index % 8
        m = int(rng.choice([1, 2, 3, 31, 32, 33, 63, 64])) if rng.random() < 0.4 else int(rng.integers(1, 65))
    if family in HAMMING and m > n and rng.random() < 0.8:  # a window longer than the text has no answer: mostly not
        m = int(rng.integers(1, n + 1))
    if family not in HAMMING or dense:  # the bound on the reference's work
        m = min(m, max(1, WORK // n))
    return min(m, MAX_M[family]), k


def _pattern(rng, family, T, S, m, k, kind):
    """The byte pattern (over S) of one of the four kinds, then 0, 1 .. k or k + 1 foreign bytes."""
    Sa = np.asarray(S, dtype=np.uint8)
    mixed = family not in HAMMING
    if kind == "window":
        at = int(rng.integers(0, max(len(T) - m, 0) + 1))
        d = max(0, int(rng.choice([0, k - 1, k, k + 1])))
        P = _fit(_edits(np.resize(T[at:at + m], m), d, rng, S, mixed), m, rng, S)
    elif kind == "periodic":
        P = np.resize(Sa[rng.integers(0, len(S), int(rng.integers(1, 6)))], m)
    elif kind == "bordered":
        lu = max(1, m // int(rng.integers(2, 5)))
        u = Sa[rng.integers(0, len(S), lu)]
        P = np.resize(np.concatenate([u, Sa[rng.integers(0, len(S), max(0, m - 2 * lu))], u]), m)
    else:
        P = Sa[rng.integers(0, len(S), m)]
    P = np.array(P, dtype=np.uint8)
    if rng.random() < (0.08 if family == "sets" else 0.2):
        u = min(m, k + 1 if rng.random() < 0.3 else int(rng.integers(1, max(k, 1) + 1)))
        foreign = [v for v in (78, 1, 254, 128, 200) if v not in S]
        P[rng.choice(m, size=u, replace=False)] = foreign[int(rng.integers(0, len(foreign)))]
    return P


def _subsets(rng, P, S, k, kind, family):
    """Per pattern position a subset of S as a bit mask over S: the singleton of the byte (nothing for a foreign byte), that
    with further members, or random with full sets and 0, 1 .. k or k + 1 empty ones."""
    code = {v: c for c, v in enumerate(S)}
    single = np.asarray([1 << code[int(b)] if int(b) in code else 0 for b in P], dtype=np.uint8)
    full = (1 << len(S)) - 1
    if kind == "singleton":
        return single
    if kind == "iupac":
        out = single.copy()
        for c in range(len(S)):
            out |= ((rng.random(len(P)) < 0.25).astype(np.uint8) << c).astype(np.uint8)
        out[single == 0] = 0
        return out
    out = rng.integers(1, full + 1, len(P)).astype(np.uint8)
    out[rng.random(len(P)) < 0.15] = full
    r = rng.random() * (0.7 if family == "sets" else 1)  # an empty set empties the set matcher's answer: rarer there
    u = 0 if r < 0.6 else min(len(P), k + 1) if r > 0.9 else min(len(P), int(rng.integers(1, max(k, 1) + 1)))
    out[rng.choice(len(P), size=u, replace=False)] = 0
    return out


def _instance(rng, P, masks, S):
    """A byte string the masks accept wherever they accept anything: the pattern's own byte where it is a member."""
    code = {v: c for c, v in enumerate(S)}
    out = np.empty(len(P), dtype=np.uint8)
    for j, (b, s) in enumerate(zip(P.tolist(), masks.tolist())):
        if b in code and s >> code[b] & 1:
            out[j] = b
        else:
            members = [v for c, v in enumerate(S) if s >> c & 1] or list(S)
            out[j] = members[int(rng.integers(0, len(members)))]
    return out


def _near_copies(rng, I, S, k, mixed, length):
    parts, have = [], 0
    while have < length:
        parts.append(_edits(I, int(rng.integers(0, k + 2)), rng, S, mixed))
        have += len(parts[-1])
    return np.concatenate(parts)[:length]


def _sub_range(rng, family, n, m, k):
    """(off, length) with off % 32 != 0, likely to end mid-dword; for the edit families a fifth of them shorter than the
    pattern: n < m <= n + k, or n + k < m."""
    off = int(rng.integers(1, n))
    if off % 32 == 0:
        off += 1 if off + 1 < n else -1
    room = n - off
    r = rng.random()
    ln = room if r < 0.25 else int(rng.integers(1, min(room, 300) + 1)) if r < 0.5 else int(rng.integers(1, room + 1))
    if family not in HAMMING and rng.random() < 0.2:
        want = m - int(rng.integers(1, k + 1)) if k >= 1 and rng.random() < 0.6 else m - k - int(rng.integers(1, 4))
        if 1 <= want <= room:
            ln = want
    if (off + ln) % 32 == 0 and ln > 1:
        ln -= 1
    return off, ln


# ---- draw --------------------------------------------------------------------------------------------------------------------

def draw(family, index, seed=SEED, small=False):
    """Case number `index` of `family` under `seed`.  small=True keeps the text to 60 symbols and the pattern to 12: the same
    kinds of input at a size where the cell-by-cell definitions can be run (tests/test_packed_fuzz.py)."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), index])
    lane, wave, _ = GEOMETRY[family]
    mixed = family not in HAMMING
    S = _values(rng, index)
    stratum, n = _length(rng, family)
    if small:
        stratum, n = "tiny", 1 + (n - 1) % 60
    text_kind = TEXT_KINDS[int(rng.integers(0, len(TEXT_KINDS)))]
    if len(S) == 1:
        text_kind = "one_value"
    if text_kind == "segments":
        def segment():
            return TEXT_KINDS[int(rng.integers(0, 5))], max(1, int([lane * rng.uniform(0.5, 3), lane * rng.uniform(6, 30), wave * rng.uniform(0.5, 1.5)][int(rng.integers(0, 3))]))
        segs = [segment()]
        while sum(ln for _, ln in segs) < n:
            segs.append(segment())
        if len(segs) == 1:  # a text too short for a second segment still gets its field
            segs = [("field", n // 2 + 1), ("uniform", n)]
        else:               # the field next to a uniform segment, both shorter than a wave's run
            at = int(rng.integers(0, len(segs) - 1))
            pair = ("field", "uniform") if rng.random() < 0.5 else ("uniform", "field")
            segs[at:at + 2] = [(kd, max(1, int(lane * rng.uniform(6, 30)))) for kd in pair]
            while sum(ln for _, ln in segs) < n:
                segs.append(segment())
        cuts = np.concatenate([[0], np.cumsum([ln for _, ln in segs])]).tolist()
        T = np.concatenate([_base(rng, S, ln, "uniform" if kd == "field" else kd) for kd, ln in segs])[:n]
        fields = [(a, min(b, n)) for (kd, _), a, b in zip(segs, cuts, cuts[1:]) if kd == "field" and a < n]
    else:
        T = _base(rng, S, n, text_kind)
        fields = []
    one_value = text_kind == "one_value"
    dense = one_value or text_kind != "uniform"
    m, k = _m_and_k(rng, family, index, n, dense)
    if small:
        m = 1 + (m - 1) % 12
    kinds = PATTERN_KINDS + ((GAPPED,) if family == "editl" else ())
    pattern_kind = kinds[int(rng.integers(0, len(kinds)))]
    gap = None
    if pattern_kind == GAPPED and small:  # a gapped pattern has at least 40 symbols
        pattern_kind = "random"
    if pattern_kind == GAPPED:
        m = min(max(m, 70), WORK // n)
        if m < 40:
            pattern_kind = "random"
        else:
            k = 29 + int(rng.integers(0, 3))
            run = k - int(rng.integers(0, 4))
            gap = (int(rng.integers(1, m - run)), run)
    # on a one-value text mostly a pattern of that value: any other byte is foreign there
    P = _pattern(rng, family, T, (int(T[0]),) if one_value and rng.random() < 0.7 else S, m, k, pattern_kind)
    if gap:
        P[gap[0]:gap[0] + gap[1]] = [v for v in (78, 1, 254, 128, 200) if v not in S][0]
    sets = family in ("sets", "sets_mis") or (family in ("edit", "editl", "align") and rng.random() < 0.5)
    set_kind = SET_KINDS[int(rng.integers(0, len(SET_KINDS)))] if sets else "singleton"
    if sets and S == ACGT and rng.random() < 0.5:  # the IUPAC letters are for these values
        set_kind = "iupac"
    if sets and gap and set_kind == "random":  # random sets would not keep the run
        set_kind = "singleton"
    masks = _subsets(rng, P, S, k, set_kind, family)
    I = _instance(rng, P, masks, S)
    ranges = [(0, n)] + ([_sub_range(rng, family, n, m, k)] if n >= 2 else [])
    if not one_value:
        for a, b in fields:
            T[a:b] = _near_copies(rng, I, S, k, mixed, b - a)
        for off, ln in ranges:
            spots = [off + int(rng.integers(0, ln)) for _ in range(40 if gap else int(rng.integers(1, 7)))] + [off, off + ln]
            for t, at in enumerate(spots):
                if gap:  # prefix and suffix with 0 .. 36 symbols between them, and a few edits
                    W = _edits(np.concatenate([I[:gap[0]], _base(rng, S, int(rng.integers(0, 37)), "uniform"), I[gap[0] + gap[1]:]]), int(rng.integers(0, 4)), rng, S, mixed)
                else:
                    W = _edits(I, int(rng.integers(0, k + 1)), rng, S, mixed)
                if len(W) > ln:
                    continue
                at = min(at, off + ln - len(W))  # the last one ends at the range's last symbol
                T[at:at + len(W)] = W
    vals = tuple(int(v) for v in np.unique(T))
    if sets:  # the subsets of S as bits over the values the text holds
        pat = np.zeros(m, dtype=np.uint8)
        for c, v in enumerate(vals):
            pat |= ((masks >> S.index(v) & 1) << c).astype(np.uint8)
    else:
        pat = P
    twin = P if sets and set_kind == "singleton" else None
    motif = None
    if sets and set_kind == "iupac" and S == ACGT and masks.all():
        motif = "".join(IUPAC[int(s)] for s in masks)
    return Case(family=family, index=index, seed=seed, S=S, vals=vals, T=T, pat=pat, sets=sets, twin=twin, motif=motif, k=k,
                all_blocks=bool(rng.integers(0, 2)), ranges=ranges, text_kind=text_kind, stratum=stratum, pattern_kind=pattern_kind,
                set_kind=set_kind, field=bool(fields) and not one_value)


def singleton_sets(P, vals):
    """The sets over `vals` that accept exactly what the byte pattern accepts: nothing for a byte the text does not hold."""
    code = {v: c for c, v in enumerate(vals)}
    return np.asarray([1 << code[int(b)] if int(b) in code else 0 for b in P], dtype=np.uint8)


# ---- the reference -------------------------------------------------------------------------------------------------------------

def reference(case, off, n):
    """(ascending positions uint64 — starts for the Hamming families, ends for the others —, distances uint8) of the case's call
    over symbols [off, off + n), by the definition the family's own module holds."""
    if case.family == "sets":
        pos = sets_gpu.by_definition(case.pat, case.T, list(case.vals), off, n)
        return pos, np.zeros(len(pos), dtype=np.uint8)
    if case.family == "mis":
        return mis_gpu.by_definition(case.pat, case.T, case.k, off, n)
    if case.family == "sets_mis":
        return sets_mis_gpu.by_definition(case.pat, case.T, case.vals, case.k, off, n)
    D = edit_row(case.m, case.accepts(), case.T, off, n)
    at = np.flatnonzero(D <= case.k)
    return (at + off).astype(np.uint64), D[at].astype(np.uint8)


def end_lists(case, r, found):
    """The three lists of ends for range number r of an align case, given the find's ends there: those ends (a seeded sample
    of ALIGN_ENDS that keeps the first and the last where they are more), a random subset of them, shuffled, with
    duplicates, and random ends of the range, which are mostly no occurrence."""
    rng = np.random.default_rng([case.seed, FAMILIES.index(case.family), case.index, 1000 + r])
    off, n = case.ranges[r]
    found = np.asarray(found, dtype=np.uint64)
    if len(found) > ALIGN_ENDS:
        keep = np.sort(rng.choice(np.arange(1, len(found) - 1), size=ALIGN_ENDS - 2, replace=False))
        found = found[np.concatenate([[0], keep, [len(found) - 1]])]
    some = found[rng.integers(0, len(found), int(rng.integers(1, ALIGN_ENDS // 2 + 1)))] if len(found) else found
    anywhere = (off + rng.integers(0, n, min(64, 2 * n))).astype(np.uint64)
    return [found, some, anywhere]


# ---- the checks on the GPU -----------------------------------------------------------------------------------------------------

class Tally:
    """What a run met: the comparisons made, the cases, and per case (lengths of its answers, distinct distances in one)."""

    def __init__(self):
        self.comparisons = 0
        self.cases = []
        self.shapes = []


def answer_shape(case):
    """(lengths of the answers over the case's ranges, the largest number of distinct distances in one of them) by the
    reference alone."""
    got = [reference(case, off, n) for off, n in case.ranges]
    return [len(p) for p, _ in got], max(len(np.unique(d)) for _, d in got)


def _calls(case, pat=None, sets=None, k=None, all_blocks=None, family=None):
    """(count(pt, off, n), find(pt, off, n, cap)) of a family's two calls for a pattern: the case's own, or another form of it."""
    import smart_amd as sa
    pat = case.pat if pat is None else pat
    sets = case.sets if sets is None else sets
    k = case.k if k is None else k
    family = family or case.family
    if family == "exact":
        return (lambda pt, off, n: sa.psearch(pat, pt, off=off, n=n)[0]), (lambda pt, off, n, cap: sa.pfind(pat, pt, off=off, n=n, cap=cap))
    if family in ("sets", "mis", "sets_mis"):
        if family == "sets":
            return (lambda pt, off, n: sa.psearch_sets(pat, pt, off=off, n=n)[0]), (lambda pt, off, n, cap: sa.pfind_sets(pat, pt, off=off, n=n, cap=cap))
        count, find = (sa.psearch_mis, sa.pfind_mis) if family == "mis" else (sa.psearch_sets_mis, sa.pfind_sets_mis)
        return (lambda pt, off, n: count(pat, pt, k, off=off, n=n)[0]), (lambda pt, off, n, cap: find(pat, pt, k, off=off, n=n, cap=cap))
    if family == "editl":
        ab = case.all_blocks if all_blocks is None else all_blocks
        count, find = (sa.psearch_sets_editl, sa.pfind_sets_editl) if sets else (sa.psearch_editl, sa.pfind_editl)
        return ((lambda pt, off, n: count(pat, pt, k, off=off, n=n, all_blocks=ab)[0]),
                (lambda pt, off, n, cap: find(pat, pt, k, off=off, n=n, cap=cap, all_blocks=ab)))
    count, find = (sa.psearch_sets_edit, sa.pfind_sets_edit) if sets else (sa.psearch_edit, sa.pfind_edit)
    return (lambda pt, off, n: count(pat, pt, k, off=off, n=n)[0]), (lambda pt, off, n, cap: find(pat, pt, k, off=off, n=n, cap=cap))


def _first_difference(a, b):
    if len(a) != len(b):
        return "lengths %d and %d" % (len(a), len(b))
    at = int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])
    return "entry %d: %s, expected %s" % (at, a[at], b[at])


def _held(calls, pt, off, n, wpos, wdist, tally, say, distances=True):
    """The count call and the find call against (wpos, wdist): the count, the list with room for it, a cap one short, cap = 0."""
    count, find = calls
    got = count(pt, off, n)
    assert got == len(wpos), "%s: the count call gives %d, expected %d" % (say, got, len(wpos))
    res = find(pt, off, n, max(len(wpos), 1))
    assert res[-1] == len(wpos) and res[0] is not None, "%s: the find call counts %d, expected %d" % (say, res[-1], len(wpos))
    assert res[0].dtype == np.uint64 and len(res[0]) == len(wpos), say
    assert np.array_equal(res[0], wpos), "%s: positions, %s" % (say, _first_difference(res[0], wpos))
    if len(res) == 3:
        assert res[1].dtype == np.uint8 and len(res[1]) == len(wpos), say
        if distances:
            assert np.array_equal(res[1], wdist), "%s: distances, %s" % (say, _first_difference(res[1], wdist))
    tally.comparisons += 2
    none = (None,) * (len(res) - 1)
    if len(wpos) >= 1:  # one short: SMARTGPU_ERR_NOMEM and the count (the binding returns None for the lists)
        short = find(pt, off, n, len(wpos) - 1)
        assert short == none + (len(wpos),), "%s: cap %d gives %s" % (say, len(wpos) - 1, short[-1])
        tally.comparisons += 1
    zero = find(pt, off, n, 0)  # cap = 0 with NULL buffers is a count
    assert zero[-1] == len(wpos) and (zero[:-1] == none if len(wpos) else all(len(x) == 0 for x in zero[:-1])), "%s: cap 0 gives %s" % (say, zero[-1])
    tally.comparisons += 1
    return res


def _same(calls, pt, off, n, wpos, wdist, tally, say, shift=0):
    """An identity: another call's count and list equal (wpos + shift, wdist) — wdist None where that call has no distances."""
    count, find = calls
    got = count(pt, off, n)
    assert got == len(wpos), "%s: the count call gives %d, the other call %d" % (say, got, len(wpos))
    res = find(pt, off, n, max(len(wpos), 1))
    assert res[-1] == len(wpos) and res[0] is not None and np.array_equal(res[0] + np.uint64(shift), wpos), "%s: positions differ" % say
    if len(res) == 3 and wdist is not None:
        assert np.array_equal(res[1], wdist), "%s: distances differ" % say
    tally.comparisons += 2


def check(case, tally):
    """Runs the case on the GPU: both calls against the reference over every range, the caps, the identities the header
    promises, and for align the three lists of ends with and without operations.  Raises AssertionError with the case's
    shape; returns nothing."""
    import smart_amd as sa
    say = case.shape()
    lengths, distinct = [], 0
    with sa.PackedText.upload(case.T) as pt:
        assert pt.symbols() == list(case.vals), say
        if case.motif is not None:
            assert np.array_equal(pt.iupac(case.motif), case.pat), say + ": iupac_sets(%s)" % case.motif
        fam = "edit" if case.family == "align" else case.family
        for r, (off, n) in enumerate(case.ranges):
            here = "%s, range %d" % (say, r)
            wpos, wdist = reference(case, off, n)
            lengths.append(len(wpos))
            distinct = max(distinct, len(np.unique(wdist)))
            _held(_calls(case, family=fam), pt, off, n, wpos, wdist, tally, here)
            # ---- the identities: no reference run
            other = singleton_sets(case.pat, case.vals) if not case.sets else case.twin
            if fam == "sets":
                if case.twin is not None:
                    _same(_calls(case, pat=case.twin, family="exact"), pt, off, n, wpos, None, tally, here + ", singleton sets against pfind")
                continue
            if other is not None:  # singleton sets give the byte call's answers, and the other way round
                _same(_calls(case, pat=other, sets=not case.sets, family={"sets_mis": "mis", "mis": "sets_mis"}.get(fam, fam)), pt, off, n, wpos, wdist,
                      tally, here + ", singleton sets against the byte pattern")
            if fam in ("mis", "sets_mis"):  # k = 0 is the exact matcher / the set matcher
                count0, find0 = _calls(case, family="exact" if fam == "mis" else "sets")
                c0 = count0(pt, off, n)
                p0 = find0(pt, off, n, max(c0, 1))[0]
                _same(_calls(case, k=0), pt, off, n, p0, np.zeros(c0, dtype=np.uint8), tally, here + ", k = 0 against the exact call")
                continue
            byte = case.pat if not case.sets else case.twin
            if byte is not None:  # edit at k = 0 is pfind + m - 1
                c0 = sa.psearch(byte, pt, off=off, n=n)[0]
                p0 = sa.pfind(byte, pt, off=off, n=n, cap=max(c0, 1))[0] + np.uint64(case.m - 1)
                _same(_calls(case, pat=byte, sets=False, k=0, family=fam), pt, off, n, p0, np.zeros(c0, dtype=np.uint8), tally, here + ", k = 0 against pfind + m - 1")
            if fam == "editl":
                _held(_calls(case, all_blocks=not case.all_blocks), pt, off, n, wpos, wdist, tally, here + ", all_blocks=%s" % (not case.all_blocks))
                if case.m <= 64 and case.k <= 7:
                    _same(_calls(case, family="edit"), pt, off, n, wpos, wdist, tally, here + ", editl against edit")
            if case.family == "align":
                call = sa.palign_sets_edit if case.sets else sa.palign_edit
                lists = end_lists(case, r, wpos)
                ends = np.concatenate(lists)
                wstarts, wd, wops = align_many(case.m, case.accepts(), case.T, ends, case.k, off)
                inside = np.isin(ends, wpos)
                assert np.array_equal(wd[inside], wdist[np.searchsorted(wpos, ends[inside])]) and (wd[~inside] == NONE_DIST).all(), here + ": the two references differ"
                at = 0
                for which, lst in zip(("the find's ends", "a shuffled subset with duplicates", "random ends of the range"), lists):
                    sl = slice(at, at + len(lst))
                    at += len(lst)
                    for ops in (True, False):
                        what = "%s, %s, ops=%s" % (here, which, ops)
                        starts, dist, words = call(case.pat, pt, case.k, lst, off=off, n=n, ops=ops)
                        assert starts.dtype == np.uint64 and dist.dtype == np.uint8, what
                        assert np.array_equal(starts, wstarts[sl]), "%s: starts, %s" % (what, _first_difference(starts, wstarts[sl]))
                        assert np.array_equal(dist, wd[sl]), "%s: distances, %s" % (what, _first_difference(dist, wd[sl]))
                        miss = ~inside[sl]
                        assert (starts[miss] == NONE_START).all() and (dist[miss] == NONE_DIST).all(), what + ": a non-occurrence without the sentinel"
                        if not ops:
                            assert words is None, what
                        else:
                            assert words.dtype == np.uint64 and words.shape == (len(lst), 3), what
                            assert np.array_equal(words, wops[sl]), "%s: operations of %s" % (what, _first_difference(words.tolist(), wops[sl].tolist()))
                            assert not words[miss].any(), what
                            hits = np.flatnonzero(~miss)
                            for x in hits[np.unique(lst[hits], return_index=True)[1]].tolist():
                                edits = replay(unpack_ops(words[x]), case.m, case.accepts(), case.T, int(starts[x]), int(lst[x]))
                                assert edits == dist[x], "%s: end %d replays to %d edits, reported %d" % (what, lst[x], edits, dist[x])
                        tally.comparisons += 1
    tally.cases.append(case)
    tally.shapes.append((lengths, distinct))


# ---- the strata ----------------------------------------------------------------------------------------------------------------

def missing_strata(family, cases, shapes):
    """What a run of `cases` (with shapes[i] = (lengths, distinct) of case i's answers, as answer_shape or Tally give them) has
    NOT met of what the fixed-seed run of a family must draw; [] when nothing is missing."""
    out = []

    def need(name, ok):
        if not ok:
            out.append(name)

    ks = {c.k for c in cases}
    if family == "editl":
        for lo, hi in ((0, 7), (8, 15), (16, 31)):
            need("a k in %d..%d" % (lo, hi), any(lo <= k <= hi for k in ks))
        need("k = 31", 31 in ks)
        need("a gapped pattern", any(c.pattern_kind == GAPPED for c in cases))
        for lo, hi in ((1, 64), (65, 128), (129, 256)):
            need("an m in %d..%d" % (lo, hi), any(lo <= c.m <= hi for c in cases))
    elif family != "sets":
        need("every k up to 7", set(range(8)) <= ks)
    need("m <= 32", any(c.m <= 32 for c in cases))
    need("m > 32", any(c.m > 32 for c in cases))
    need("1, 2, 3 and 4 values", {len(c.vals) for c in cases} >= {1, 2, 3, 4})
    need("a range with off % 32 != 0", any(off % 32 for c in cases for off, _ in c.ranges))
    need("a range that ends mid-dword", any((off + n) % 32 for c in cases for off, n in c.ranges[1:]))
    need("every text kind", {c.text_kind for c in cases} >= set(TEXT_KINDS))
    need("every length stratum", {c.stratum for c in cases} >= {"tiny", "around", "large"})
    need("every pattern kind", {c.pattern_kind for c in cases} >= set(PATTERN_KINDS))
    need("a segmented text with a field of near-copies", any(c.field for c in cases))
    need("k >= m", family == "sets" or any(c.k >= c.m for c in cases))
    if family in ("edit", "editl", "align"):
        need("both forms of the pattern", {c.sets for c in cases} == {True, False})
        need("a range with n < m <= n + k", any(n < c.m <= n + c.k for c in cases for _, n in c.ranges))
        need("a range with n + k < m", any(n + c.k < c.m for c in cases for _, n in c.ranges))
    if family != "mis":
        need("every kind of sets", {c.set_kind for c in cases if c.sets} >= set(SET_KINDS))
        need("an IUPAC motif", any(c.motif is not None for c in cases))
    need("a short cap", any(any(ln) for ln, _ in shapes))
    need("an empty answer", any(not all(ln) for ln, _ in shapes))
    need("half of the cases with an answer", 2 * sum(any(ln) for ln, _ in shapes) >= len(cases))
    if family != "sets":  # the set matcher has no distances
        need("a tenth of the cases with two distances", 10 * sum(d >= 2 for _, d in shapes) >= len(cases))
    return out
