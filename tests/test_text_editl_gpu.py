"""Edit distance for LONG patterns on BYTE texts on the GPU (smartgpu_search_editl64, smartgpu_find_editl64 and their classes
forms; text_editl_scan and text_editl_find of k_teditl.hip) against the by-definition oracle of tests/test_packed_edit.py
(edit_row: Sellers' programme on the range alone).  Every comparison is exact equality, of the count, the ends AND the
distances.

The oracle's row D(e) does not depend on k and costs m vector passes over n, so every (alphabet, n, m) builds ONE text,
planted with copies of the pattern that carry 0 .. 32 edits, uploads it once, runs the oracle once and checks the calls at
every k against that row.  The sizes are the smallest at which a piece (128 bytes), a run (512), a wave's 32 KiB and a
super-tile (128 KiB) have a neighbour; 2^20 + 3 bytes — eight super-tiles and a ragged one — run for two lengths on two
alphabets only."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import smart_amd  # noqa: E402
from smart_amd import (SmartGpuError, byte_classes, engine, find_edit, find_editl, find_editl_classes, search_edit, search_editl,  # noqa: E402
                       search_editl_classes)

from test_packed_edit import byte_accepts, edit_row  # noqa: E402
from test_text_edit_gpu import ALPHABETS, check, class_accepts, draw, english, uploaded  # noqa: E402
from tiled_oracle import edited  # noqa: E402

ERR_NOMEM = -5
PIECE, RUN, WAVE_RUN, SUPER = 128, 512, 32768, 131072  # what a lane walks per trip and owns, a wave's and a workgroup's runs (k_teditl.hip)
MS = (1, 64, 65, 128, 129, 255, 256)
KS = (0, 1, 7, 8, 16, 31)
NS = (1, 2, 127, 128, 129, 511, 512, 513, 32767, 32768, 32769, 131071, 131072, 131073)
EDITS = (0, 1, 2, 7, 8, 9, 16, 17, 31, 32)  # k and k + 1 for every k of the grid
SEAMS = (127, 128, 511, 512, 513, 32768, 131072)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert smart_amd.device_count() > 0, "no HIP device: " + smart_amd.lib().smartgpu_last_error().decode()


def plant(T, P, vals, ds, rng):
    """Copies of P with d edits of mixed kinds for d in ds, spread over T where T has the room; returns how many went in."""
    n, m, done = len(T), len(P), 0
    for t, d in enumerate(ds):
        try:
            W = edited(P, d, rng, vals, True) if d else P.copy()
        except ValueError:  # the pattern has fewer than d places to edit
            continue
        a = (t + 1) * n // (len(ds) + 2)
        if n < (len(ds) + 2) * (m + 40) or a + len(W) > n:
            continue
        T[a:a + len(W)] = W
        done += 1
    return done


def check_bytes(text, P, row, k, off=0, n=None, all_blocks=False):
    return check(text, row, k, off, n, lambda t, k, off, n: search_editl(P, t, k, off=off, n=n, all_blocks=all_blocks),
                 lambda t, k, off, n, cap: find_editl(P, t, k, off=off, n=n, cap=cap, all_blocks=all_blocks), ("bytes", len(P), all_blocks))


def grid(name, ns, ms, rng, both):
    """Every m of ms, k of KS and n of ns on one alphabet; with `both` every cell with all_blocks as well."""
    cases = hits = planted = 0
    for n in ns:
        for m in ms:
            T, vals = draw(name, n, rng)
            if n >= m:
                a = int(rng.integers(0, n - m + 1))
                P = T[a:a + m].copy()
            else:
                P = draw(name, m, rng)[0]
            planted += plant(T, P, vals, EDITS, rng)
            row = edit_row(m, byte_accepts(P), T)
            with uploaded(T) as text:
                for k in KS:
                    hits += check_bytes(text, P, row, k)
                    if both:
                        check_bytes(text, P, row, k, all_blocks=True)
                    cases += 1
    return cases, hits, planted


# ---- alphabets x lengths x k x sizes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ALPHABETS))
def test_alphabets_lengths_and_k(name):
    """The whole grid on one alphabet.  The pattern is cut from the text (drawn from the alphabet where the text is shorter) and
    copies with 0 .. 32 edits of mixed kinds are planted where the text has the room.  On ACGT every cell runs with all_blocks
    too, against the same row."""
    rng = np.random.default_rng(5000 + list(ALPHABETS).index(name))
    cases, hits, planted = grid(name, NS, MS, rng, name == "acgt")
    assert cases == len(NS) * len(MS) * len(KS) and planted >= 6 * 6 * 5 and hits > cases


@pytest.mark.parametrize("name", ["acgt", "all256"])
def test_eight_super_tiles_and_a_ragged_one(name):
    rng = np.random.default_rng(5100 + len(name))
    cases, hits, planted = grid(name, (2**20 + 3,), (65, 256), rng, name == "acgt")
    assert cases == 2 * len(KS) and planted == 2 * len(EDITS) and hits > cases


# ---- seams -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 300])
@pytest.mark.parametrize("m", [65, 256])
def test_copies_that_end_at_the_seams(m, off):
    """Copies of the pattern with 0 .. k + 1 mixed edits that END at offsets 127, 128 (two pieces), 511, 512, 513 (two runs),
    32768 (two waves) and 131072 (two super-tiles) of the range, over 256 values: nothing but the copies is near.  A copy that
    does not fit between the range's first byte and its seam is cut at the front: on the range alone it is that much further."""
    rng = np.random.default_rng(5200 + m + off)
    vals = tuple(range(256))
    n = SUPER + 2 * RUN + 77
    P = rng.integers(0, 256, m).astype(np.uint8)
    rounds = ((127, 512, 32768, 131072), (128, 513), (511,))  # (copies that end a byte apart would overwrite each other)
    assert sorted(s for r in rounds for s in r) == sorted(SEAMS)
    t = whole = 0
    for seams in rounds:
        T = rng.integers(0, 256, off + n).astype(np.uint8)
        placed = []
        for seam in seams:
            d = EDITS[(t + m) % len(EDITS)]
            t += 1
            W = edited(P, d, rng, vals, True) if d else P.copy()
            e = off + seam
            cut = len(W) > seam + 1
            W = W[-min(len(W), seam + 1):]
            T[e + 1 - len(W):e + 1] = W
            placed.append((e, d, cut))
        row = edit_row(m, byte_accepts(P), T, off, n)
        # (the inputs) a whole copy with d edits ends at most d from the pattern
        assert all(row[e - off] <= d for e, d, cut in placed if not cut)
        whole += sum(not cut for e, d, cut in placed)
        with uploaded(T) as text:
            for k in KS:
                got = check_bytes(text, P, row, k, off, n)
                assert got >= sum(1 for e, d, cut in placed if not cut and d <= k)
                check_bytes(text, P, row, k, off, n, all_blocks=True)
    assert whole >= len(SEAMS) - 2


# ---- ranges ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [300, 512 * 5 + 77, 131072 - 100, 512 * 3 + 500])
def test_ranges_read_nothing_before_their_first_byte(off):
    """`off` lies in the middle of a piece; with 512 * 3 + 500 the range's second run begins 12 bytes behind it, so the lanes of
    its first TWO runs start clipped.  A copy of the pattern lies across `off`, its first h bytes just BEFORE the range: on the
    range alone its end is h edits away — a kernel that reads a distance out of bytes before the range reports 0.  Once with a
    range that ends mid-run, once with one that ends with the text."""
    rng = np.random.default_rng(5300 + off)
    n_text = off + SUPER + 3 * RUN + 77
    for m, k, h in ((100, 7, 2), (256, 31, 9), (256, 31, 100), (65, 0, 1)):
        T = rng.integers(0, 256, n_text).astype(np.uint8)
        P = rng.integers(0, 256, m).astype(np.uint8)
        T[off - h:off - h + m] = P
        T[off + 5000:off + 5000 + m] = P
        whole = edit_row(m, byte_accepts(P), T, off - h, m + 10)
        assert whole[m - 1] == 0  # (the inputs) on the text the copy is exact
        with uploaded(T) as text:
            for n in (n_text - off - RUN - 37, n_text - off):
                assert (off + n) % RUN != 0 or off + n == n_text
                row = edit_row(m, byte_accepts(P), T, off, n)
                e = m - 1 - h  # the copy's end, relative to off: h edits away on the range alone
                assert row[e] == h
                assert check_bytes(text, P, row, k, off, n) >= 1 + (h <= k)
                check_bytes(text, P, row, k, off, n, all_blocks=True)


def test_empty_and_short_ranges():
    rng = np.random.default_rng(5400)
    T = rng.integers(0, 4, 3000).astype(np.uint8)
    P = T[1000:1200].copy()
    with uploaded(T) as text:
        # n = 0
        assert search_editl(P, text, 5, off=700, n=0) == 0
        ends, dist = find_editl(P, text, 5, off=700, n=0)
        assert len(ends) == 0 and len(dist) == 0
        # n + k < m: nothing, without a launch
        assert search_editl(P, text, 31, off=1000, n=168) == 0
        ends, dist = find_editl(P, text, 31, off=1000, n=168)
        assert len(ends) == 0 and len(dist) == 0
        # m > n with n + k >= m: the range is the pattern without its last 31, 20, 1 bytes
        for short, k in ((31, 31), (20, 31), (20, 20), (1, 1), (1, 0)):
            n = 200 - short
            row = edit_row(200, byte_accepts(P), T, 1000, n)
            assert row[-1] == short
            assert check_bytes(text, P, row, k, 1000, n) == sum(row <= k)
        # a range outside a real text is refused, nothing written
        c = ctypes.c_uint64(77)
        L = engine.lib()
        assert L.smartgpu_search_editl64(P.ctypes.data, 200, 3, 0, text._h, 1, len(T), ctypes.byref(c), None, None) == -3 and c.value == 77
        assert "outside the text" in L.smartgpu_last_error().decode()


def test_k_at_least_m_reports_every_end_with_its_distance():
    rng = np.random.default_rng(5500)
    n = WAVE_RUN + RUN + 5
    T = np.asarray(tuple(b"ACDEFGHIKLMNPQRSTVWY"), dtype=np.uint8)[rng.integers(0, 20, n)]
    with uploaded(T) as text:
        for m, k in ((3, 3), (20, 31), (31, 31), (1, 16)):
            P = T[100:100 + m].copy()
            assert check_bytes(text, P, edit_row(m, byte_accepts(P), T), k) == n


# ---- identities ------------------------------------------------------------------------------------------------------------

def test_short_patterns_equal_the_short_calls():
    """For m <= 64 and k <= 7 the answers are find_edit's and search_edit's, from the other kernel."""
    E = english()[:SUPER + 4321]
    rng = np.random.default_rng(5600)
    A = np.asarray((65, 67, 71, 84), dtype=np.uint8)[rng.integers(0, 4, SUPER + 4321)]
    for T in (E, A):
        with uploaded(T) as text:
            for m, k in ((1, 0), (8, 1), (20, 3), (32, 7), (33, 2), (64, 7)):
                P = T[7000:7000 + m].copy()
                for off, n in ((0, len(T)), (300, 40000), (RUN * 5 + 77, len(T) - RUN * 5 - 77)):
                    want, wdist = find_edit(P, text, k, off=off, n=n, cap=n)
                    ends, dist = find_editl(P, text, k, off=off, n=n, cap=n)
                    assert len(want) > 0 and np.array_equal(ends, want) and np.array_equal(dist, wdist), (m, k, off)
                    assert search_editl(P, text, k, off=off, n=n) == search_edit(P, text, k, off=off, n=n) == len(want)
                    ends, dist = find_editl(P, text, k, off=off, n=n, cap=n, all_blocks=True)
                    assert np.array_equal(ends, want) and np.array_equal(dist, wdist), (m, k, off)


def test_classes_singletons_ignore_case_and_rows_by_hand():
    E = english()[:SUPER + 1001]
    fold = np.arange(256, dtype=np.uint8)
    fold[65:91] += 32
    with uploaded(E) as text:
        # one bit per row: the byte pattern's answers
        for a, m, k in ((5000, 100, 7), (70000, 256, 31), (200, 65, 8)):
            P = E[a:a + m].copy()
            ends, dist = find_editl(P, text, k, cap=len(E))
            cends, cdist = find_editl_classes(byte_classes(P), text, k, cap=len(E))
            assert len(ends) > 0 and np.array_equal(ends, cends) and np.array_equal(dist, cdist)
            assert search_editl_classes(byte_classes(P), text, k) == len(ends)
        # ignore_case: the oracle over class_accepts, and over the folded comparison
        for a, m, k in ((12345, 100, 7), (40000, 150, 16), (90001, 256, 31)):
            P = E[a:a + m].copy()
            swapped = np.where(((P >= 65) & (P <= 90)) | ((P >= 97) & (P <= 122)), P ^ 0x20, P).astype(np.uint8)
            rows = byte_classes(swapped, ignore_case=True)
            row = edit_row(m, class_accepts(rows), E)
            assert np.array_equal(row, edit_row(m, lambda i, R, Q=swapped: fold[R] == fold[Q[i]], E)) and row[a + m - 1] == 0
            for kk in (0, k):
                got = check(text, row, kk, count=lambda t, k, off, n: search_editl_classes(rows, t, k, off=off, n=n),
                            find=lambda t, k, off, n, cap: find_editl_classes(rows, t, k, off=off, n=n, cap=cap), what=("ignore_case", m))
                assert got >= 1
                check(text, row, kk, count=lambda t, k, off, n: search_editl_classes(rows, t, k, off=off, n=n, all_blocks=True),
                      find=lambda t, k, off, n, cap: find_editl_classes(rows, t, k, off=off, n=n, cap=cap, all_blocks=True), what=("ignore_case", m, "all"))
        # rows by hand, 70 of them: an EMPTY row (accepts nothing: one edit at least), FULL rows, vowels, blanks
        rows = np.zeros((70, 32), dtype=np.uint8)
        for j in range(70):
            members = (b"tT", b"aeiou", None, b" ,.;:", b"aeiouAEIOU", None, b"hH")[j % 7] if j != 40 else b""
            for v in (range(256) if members is None else members):
                rows[j, v >> 3] |= 1 << (v & 7)
        assert not rows[40].any() and (rows[2] == 255).all()
        row = edit_row(70, class_accepts(rows), E)
        nearest = int(row.min())
        assert 1 <= nearest <= 31
        for k in (0, nearest - 1, nearest, 31):
            got = check(text, row, k, count=lambda t, k, off, n: search_editl_classes(rows, t, k, off=off, n=n),
                        find=lambda t, k, off, n, cap: find_editl_classes(rows, t, k, off=off, n=n, cap=cap), what="by hand")
            assert (got == 0) == (k < nearest)


# ---- cap -------------------------------------------------------------------------------------------------------------------

def test_cap_count_and_missing_buffers():
    rng = np.random.default_rng(5700)
    T = np.asarray((65, 67, 71, 84), dtype=np.uint8)[rng.integers(0, 4, 50000)]
    m, k = 100, 31
    P = T[777:777 + m].copy()
    row = edit_row(m, byte_accepts(P), T)
    wends = np.flatnonzero(row <= k).astype(np.uint64)
    total = len(wends)
    assert total >= 50
    L = engine.lib()
    with uploaded(T) as text:
        ends = np.full(total + 4, 7, dtype=np.uint64)
        dist = np.full(total + 4, 9, dtype=np.uint8)
        c = ctypes.c_uint64(0)
        # one short: the true count, SMARTGPU_ERR_NOMEM, nothing behind ends[cap] touched
        assert L.smartgpu_find_editl64(P.ctypes.data, m, k, 0, text._h, 0, len(T), ends.ctypes.data, dist.ctypes.data, total - 1, ctypes.byref(c)) == ERR_NOMEM
        assert c.value == total and "room for %d" % (total - 1) in L.smartgpu_last_error().decode()
        assert (ends[total - 1:] == 7).all() and (dist[total - 1:] == 9).all()
        with pytest.raises(SmartGpuError, match="%d occurrences" % total):
            find_editl(P, text, k, cap=total - 1)
        # cap = 0 with NULL buffers is a count
        c = ctypes.c_uint64(0)
        assert L.smartgpu_find_editl64(P.ctypes.data, m, k, 1, text._h, 0, len(T), None, None, 0, ctypes.byref(c)) == ERR_NOMEM and c.value == total
        # exactly enough, distances == NULL: the ends, and nothing behind them
        c = ctypes.c_uint64(0)
        assert L.smartgpu_find_editl64(P.ctypes.data, m, k, 0, text._h, 0, len(T), ends.ctypes.data, None, total, ctypes.byref(c)) == 0
        assert c.value == total and np.array_equal(ends[:total], wends) and (ends[total:] == 7).all() and (dist == 9).all()
        # the classes form takes the same paths
        rows = byte_classes(P)
        c = ctypes.c_uint64(0)
        assert L.smartgpu_find_editl_classes64(rows.ctypes.data, m, k, 0, text._h, 0, len(T), ends.ctypes.data, dist.ctypes.data, total - 1, ctypes.byref(c)) == ERR_NOMEM
        assert c.value == total
        # the times of a count
        pre, run = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        assert L.smartgpu_search_editl64(P.ctypes.data, m, k, 0, text._h, 0, len(T), ctypes.byref(c), ctypes.byref(pre), ctypes.byref(run)) == 0
        assert c.value == total and pre.value >= 0.0 and run.value > 0.0


# ---- block switching -------------------------------------------------------------------------------------------------------

def test_planted_prefixes_switch_blocks_on_and_off():
    """Prefixes of 100 and 200 bytes of a 256-byte pattern, each followed by noise, at k = 7: the oracle alone shows values
    <= k in rows >= 33 (the cut-off must switch further blocks on) and no occurrence (it must get the rest right)."""
    rng = np.random.default_rng(5800)
    m, k = 256, 7
    n = SUPER + WAVE_RUN + 777
    T = rng.integers(0, 256, n).astype(np.uint8)
    P = rng.integers(0, 256, m).astype(np.uint8)
    at = []
    for t, a in enumerate((RUN - 60, 40 * RUN + 300, WAVE_RUN - 150, SUPER - 120, SUPER + 3 * RUN + 1)):
        ln = (100, 200)[t % 2]
        T[a:a + ln] = P[:ln]
        T[a + ln] = P[ln] ^ 0x55
        at.append((a, ln))
    # (the inputs) from the oracle alone: deep rows reach values <= k, the last row never does
    for rows in (33, 100, 200):
        sub = edit_row(rows, byte_accepts(P[:rows]), T)
        assert sub.min() == 0 and all(sub[a + rows - 1] == 0 for a, ln in at if ln >= rows)
    row = edit_row(m, byte_accepts(P), T)
    assert row.min() > k
    with uploaded(T) as text:
        assert check_bytes(text, P, row, k) == 0
        assert check_bytes(text, P, row, k, all_blocks=True) == 0
        # and with one whole copy behind the prefixes, at 31 edits' reach
        W = edited(P, 5, rng, tuple(range(256)), True)
    T[SUPER + 9 * RUN:SUPER + 9 * RUN + len(W)] = W
    row = edit_row(m, byte_accepts(P), T)
    with uploaded(T) as text:
        assert check_bytes(text, P, row, k) >= 1
        assert check_bytes(text, P, row, 31) >= 1
