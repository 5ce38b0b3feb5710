// packed_alignl_check.cpp — starts and alignments of LONG edit-distance occurrences on packed texts on the CPU
// (tests/test_packed_alignl.py builds it with AddressSanitizer and UBSan and runs it): smart_amd/csrc/alignl_band.hpp run as
// planes_editl_align (k_palignl.hip) runs it — 64 lanes, one per diagonal, stepped over the anti-diagonals with each lane's
// neighbours taken from the previous step's values; the four masks of the REVERSED pattern from editl_peq_pattern /
// editl_peq_sets (peditl_host.hpp); every symbol's code taken by shift from the wave's window of 10 aligned dwords per plane
// that ends with plane dword e >> 5 (palignl.hpp's geometry); min(m + k, e - off + 1) columns; decisions packed sixteen rows
// per dword as [row / 16][lane]; the key reduction; the wave-uniform walk with lane t / 32 holding word t / 32 — against a
// scalar full-matrix DP of the suffix distances written out here in forward coordinates: the definition of
// smartgpu_palign_editl64 (include/smartgpu.h).  The planes have GUARD words: what lies below dword 0, and the bits of the last
// dword beyond the text, are random, so a band that consumed one of them would disagree with the definition; a read beyond
// the guard, or above dword e >> 5, is refused outright.
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
#include <hip/hip_runtime_api.h>  // palignl.hpp names hipError_t and hipStream_t in its launcher's type; nothing of HIP is called

#include "palignl.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int g_cases = 0, g_failures = 0;

void check(bool ok, const char* what, unsigned a = 0, unsigned b = 0, unsigned c = 0, unsigned d = 0)
{
    ++g_cases;
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s (%u, %u, %u, %u)\n", what, a, b, c, d);
}

unsigned long long g_x = 88172645463325252ull;
unsigned rnd(unsigned mod)
{
    g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17;
    return static_cast<unsigned>((g_x >> 11) % mod);
}

// The text as the device holds it: codes as bit planes, 32 symbols per dword, with kGuard random dwords below dword 0 of
// each plane and random bits behind symbol n - 1 in the last dword.  dword(b, x) is plane b's dword x, x >= -kGuard; .at()
// refuses everything else.
constexpr long long kGuard = sg::kPAlignlWinDw - 1;
struct Planes {
    std::vector<uint32_t> store[2];
    size_t n;
    int planes;
    Planes(const std::vector<uint8_t>& codes, int planes_) : n(codes.size()), planes(planes_)
    {
        const size_t dwords = (n + 31) / 32;
        for (int b = 0; b < 2; ++b) {
            store[b].resize(static_cast<size_t>(kGuard) + dwords);
            for (auto& w : store[b]) w = (rnd(65536) << 16) | rnd(65536);
            for (size_t s = 0; s < n; ++s) {
                uint32_t& w = store[b][static_cast<size_t>(kGuard) + s / 32];
                w = (w & ~(1u << (s % 32))) | static_cast<uint32_t>(codes[s] >> b & 1) << (s % 32);
            }
        }
    }
    uint32_t dword(int b, long long x) const { return store[b].at(static_cast<size_t>(kGuard + x)); }
};

struct Result {
    bool hit = false;      // D(e) <= k
    size_t start = 0;
    int dist = 0;
    std::vector<uint8_t> ops;
    bool operator==(const Result& o) const { return hit == o.hit && (!hit || (start == o.start && dist == o.dist && ops == o.ops)); }
};

// pattern position i accepts code c: bit c of accepts[i] (a plain pattern: one bit, or none for a byte the text does not hold)
using Accepts = std::vector<uint8_t>;

// ---- the definition: S[i][p] = ed(P[i..m), T[p..e]) for lo <= p <= e + 1, lo = max(off, e + 1 - (m + k)) ----
Result scalar_align(const Accepts& A, const std::vector<uint8_t>& T, size_t off, size_t e, unsigned k)
{
    const size_t m = A.size();
    const size_t lo = e + 1 - off > m + k ? e + 1 - (m + k) : off;
    const size_t W = e + 1 - lo;  // symbols lo .. e; column index c = p - lo, 0 .. W (W: the empty suffix)
    std::vector<int> S((m + 1) * (W + 1));
    auto at = [&](size_t i, size_t c) -> int& { return S[i * (W + 1) + c]; };
    for (size_t c = 0; c <= W; ++c) at(m, c) = static_cast<int>(W - c);
    for (size_t i = m; i-- > 0;) {
        at(i, W) = static_cast<int>(m - i);
        for (size_t c = W; c-- > 0;) {
            const int sub = at(i + 1, c + 1) + (A[i] >> T[lo + c] & 1 ? 0 : 1);
            at(i, c) = std::min(sub, std::min(at(i + 1, c) + 1, at(i, c + 1) + 1));
        }
    }
    Result r;
    size_t best = W;  // the LARGEST start among the minimisers
    for (size_t c = W; c-- > 0;)
        if (at(0, c) < at(0, best)) best = c;
    r.dist = at(0, best);
    r.hit = r.dist <= static_cast<int>(k);
    r.start = lo + best;
    if (!r.hit) return r;
    size_t i = 0, c = best;
    while (i < m || c < W) {
        if (i < m && c < W) {
            const bool acc = A[i] >> T[lo + c] & 1;
            if (at(i + 1, c + 1) + (acc ? 0 : 1) == at(i, c)) {
                r.ops.push_back(acc ? 0 : 1);
                ++i; ++c;
                continue;
            }
        }
        if (i < m && at(i + 1, c) + 1 == at(i, c)) {
            r.ops.push_back(3);
            ++i;
        } else {
            r.ops.push_back(2);
            ++c;
        }
    }
    return r;
}

// The kernel's masks: of the reversed bytes through editl_peq_pattern, or of the reversed sets through editl_peq_sets
struct Masks {
    uint32_t peq[4][sg::kEditlWords];
};
Masks reversed_masks(const std::vector<uint8_t>& pat, bool sets, const uint8_t values[4], int nvalues)
{
    const uint32_t m = static_cast<uint32_t>(pat.size());
    std::vector<uint8_t> rev(pat.rbegin(), pat.rend());
    Masks q;
    if (sets) {
        if (sg::editl_peq_sets(nvalues, rev.data(), m, q.peq) != -1) check(false, "a set names a code the text does not hold");
    } else {
        sg::editl_peq_pattern(values, nvalues, rev.data(), m, q.peq);
    }
    return q;
}

// ---- the same through alignl_band.hpp, as the wave runs it ----
Result band_align(const Masks& q, uint32_t m, const Planes& text, size_t off, size_t e, unsigned k, bool* packing_ok)
{
    constexpr uint32_t kLanes = sg::kAlignlLanes, kDw = sg::kPAlignlWinDw;
    uint32_t win[2 * kDw] = {};
    const long long first = sg::palignl_window_first(e);
    for (int b = 0; b < text.planes; ++b)
        for (uint32_t w = 0; w < kDw; ++w) win[b * kDw + w] = text.dword(b, first + w);
    if (first + kDw - 1 != static_cast<long long>(e >> 5)) *packing_ok = false;  // nothing above dword e >> 5
    const uint32_t ncols = sg::talign_columns(e, off, m + k);
    const uint32_t* masks = &q.peq[0][0];  // the kernel's LDS copy: [code][word]

    std::vector<uint32_t> dec(sg::kAlignlDecDw * kLanes, 0xffffffffu);  // (what an earlier occurrence left: never read on a hit's path)
    int val[kLanes];
    uint32_t acc[kLanes], key[kLanes];
    for (uint32_t l = 0; l < kLanes; ++l) {
        val[l] = sg::kAlignlBig;
        acc[l] = 0;
        key[l] = sg::kAlignlKeyNone;
    }
    for (uint32_t step = 0; step <= m + ncols; ++step) {
        int up[kLanes], left[kLanes];  // the wave shifts: every lane, before any lane of this step writes
        for (uint32_t l = 0; l < kLanes; ++l) {
            up[l] = l + 1 < kLanes ? val[l + 1] : 0;
            left[l] = l > 0 ? val[l - 1] : 0;
        }
        for (uint32_t l = 0; l < kLanes; ++l) {
            const int d = sg::alignl_diag(l);
            const bool live = sg::alignl_live(d, k), up_ok = live && sg::alignl_live(d + 1, k), left_ok = live && sg::alignl_live(d - 1, k);
            uint32_t i, j;
            if (!(live && sg::alignl_step_cell(step, d, m, ncols, &i, &j))) continue;
            if (i + j != step || static_cast<int>(j) - static_cast<int>(i) != d) *packing_ok = false;
            int nv;
            if (i == 0) {
                nv = static_cast<int>(j);
            } else if (j == 0) {
                nv = static_cast<int>(i);
            } else {
                const uint32_t wb = sg::palignl_window_bit(e, j);
                // the issue's statement of the same bit: symbol e - j + 1, bit & 31 of plane dword >> 5, relative to `first`
                const size_t sym = e - j + 1;
                if ((wb & 31u) != (sym & 31u) || static_cast<long long>(wb >> 5) != static_cast<long long>(sym >> 5) - first || (wb >> 5) >= kDw) *packing_ok = false;
                uint32_t code = (win[wb >> 5] >> (wb & 31u)) & 1u;
                if (text.planes == 2) code |= ((win[kDw + (wb >> 5)] >> (wb & 31u)) & 1u) << 1;
                const uint32_t index = sg::palignl_peq_index(i, code);
                if (index >= 4 * sg::kEditlWords) *packing_ok = false;
                const uint32_t miss = sg::alignl_miss(i, masks[index % (4 * sg::kEditlWords)]);
                const sg::AlignlCell c = sg::alignl_cell(val[l], up_ok ? up[l] : sg::kAlignlBig, left_ok ? left[l] : sg::kAlignlBig, miss);
                nv = c.value;
                acc[l] |= c.op << sg::alignl_dec_shift(i);
                if (sg::alignl_dec_flush(i, j, m, ncols)) {
                    dec.at(sg::alignl_dec_dword(i) * kLanes + l) = acc[l];
                    acc[l] = 0;
                }
            }
            val[l] = nv;
            if (i == m) key[l] = sg::alignl_key(nv, j);
        }
    }
    const uint32_t best = *std::min_element(key, key + kLanes);
    const uint32_t dist = sg::alignl_key_dist(best), J = sg::alignl_key_j(best);
    Result r;
    r.dist = static_cast<int>(dist);
    r.hit = dist <= k;
    if (!r.hit) return r;
    r.start = e + 1 - J;
    unsigned long long word[kLanes] = {};
    uint32_t i = m, j = J, t = 0;
    while (i > 0 || j > 0) {
        uint32_t dec2 = 0;
        if (i > 0 && j > 0) {
            if (sg::alignl_dec_lane(i, j) != static_cast<uint32_t>(static_cast<int>(j) - static_cast<int>(i) + sg::kAlignlMid)) *packing_ok = false;  // inside the band
            dec2 = dec.at(sg::alignl_dec_dword(i) * kLanes + sg::alignl_dec_lane(i, j)) >> sg::alignl_dec_shift(i) & 3u;
        }
        const uint32_t op = sg::alignl_walk_step(&i, &j, dec2);
        for (uint32_t l = 0; l < kLanes; ++l) word[l] |= l == sg::alignl_op_word(t) ? sg::alignl_op_bits(t, op) : 0ull;
        ++t;
    }
    word[sg::kAlignlOpsWords - 1] = t;
    const uint32_t L = t;
    if (L > sg::kAlignlMaxOps || word[9] != L) *packing_ok = false;
    for (uint32_t u = 0; u < 32 * (sg::kAlignlOpsWords - 1); ++u) {
        const uint8_t op = static_cast<uint8_t>(word[u / 32] >> (2 * (u % 32)) & 3);
        if (u < L) r.ops.push_back(op);
        else if (op) *packing_ok = false;  // every unused bit is 0
    }
    return r;
}

struct Seen {
    unsigned hits = 0, misses = 0, phases = 0, clipped = 0, below = 0;  // phases: bit e % 32; below: a window that begins below dword 0
    std::vector<bool> ncols;                                             // ncols[c]: a band of c columns was run at k = 7
};

bool end_agrees(const Masks& q, const Accepts& A, const std::vector<uint8_t>& T, const Planes& text, size_t off, size_t e, unsigned k, Seen* seen)
{
    bool packing = true;
    const Result want = scalar_align(A, T, off, e, k);
    const Result got = band_align(q, static_cast<uint32_t>(A.size()), text, off, e, k, &packing);
    ++(want.hit ? seen->hits : seen->misses);
    seen->phases |= 1u << (e & 31);
    if (e - off + 1 < A.size() + k) ++seen->clipped;
    if (sg::palignl_window_first(e) < 0) ++seen->below;
    if (k == 7) seen->ncols.at(sg::talign_columns(e, off, static_cast<uint32_t>(A.size()) + k)) = true;
    if (!(want == got) || !packing)
        std::printf("  e = %zu off = %zu: want hit %d start %zu dist %d L %zu, got hit %d start %zu dist %d L %zu, packing %d\n", e, off, (int)want.hit,
                    want.start, want.dist, want.ops.size(), (int)got.hit, got.start, got.dist, got.ops.size(), (int)packing);
    return want == got && packing;
}

// a copy of P (codes) with g edits of mixed kinds at random places
std::vector<uint8_t> edited(const std::vector<uint8_t>& P, unsigned g, unsigned nvalues)
{
    std::vector<uint8_t> c = P;
    for (unsigned x = 0; x < g; ++x) {
        const unsigned kind = rnd(3);
        const uint8_t v = static_cast<uint8_t>(rnd(nvalues));
        if (kind == 0 && !c.empty()) c[rnd(static_cast<unsigned>(c.size()))] = v;
        else if (kind == 1) c.insert(c.begin() + rnd(static_cast<unsigned>(c.size()) + 1), v);
        else if (!c.empty()) c.erase(c.begin() + rnd(static_cast<unsigned>(c.size())));
    }
    return c;
}

void align_cases()
{
    const unsigned ms[] = {1, 31, 32, 33, 64, 65, 128, 129, 255, 256};
    const uint8_t letters[4] = {'A', 'C', 'G', 'T'};
    const size_t off = 37;  // a range that starts inside the text, mid-dword
    for (unsigned m : ms) {
        Seen seen;
        seen.ncols.assign(m + 7 + 1, false);
        for (unsigned nvalues : {1u, 2u, 3u, 4u}) {
            uint8_t values[4] = {255, 255, 255, 255};
            for (unsigned v = 0; v < nvalues; ++v) values[v] = letters[v];
            const int planes = nvalues > 2 ? 2 : 1;
            for (bool sets : {false, true}) {
                // the pattern as codes (what the planted copies are cut from), and what the call receives: bytes, or sets
                // that hold the code, sometimes a second one, sometimes every one; one position of the set form is EMPTY
                std::vector<uint8_t> Pc(m), pat(m);
                Accepts A(m);
                for (unsigned i = 0; i < m; ++i) {
                    Pc[i] = static_cast<uint8_t>(rnd(nvalues));
                    if (sets) {
                        const unsigned kind = rnd(8);
                        A[i] = static_cast<uint8_t>(kind == 0 ? (1u << nvalues) - 1u : kind == 1 ? (1u << Pc[i]) | (1u << rnd(nvalues)) : 1u << Pc[i]);
                        pat[i] = A[i];
                    } else {
                        A[i] = static_cast<uint8_t>(1u << Pc[i]);
                        pat[i] = values[Pc[i]];
                    }
                }
                if (sets && m > 2) pat[m / 2] = A[m / 2] = 0;
                const Masks q = reversed_masks(pat, sets, values, static_cast<int>(nvalues));
                for (unsigned k : {0u, 1u, 7u, 8u, 31u}) {
                    // the text: filler, then planted copies with 0 .. k + 1 mixed edits, a few filler symbols between them
                    std::vector<uint8_t> T(off + 3);
                    for (auto& c : T) c = static_cast<uint8_t>(rnd(nvalues));
                    std::vector<size_t> planted;
                    for (unsigned g = 0; g <= k + 1; ++g) {
                        const std::vector<uint8_t> copy = edited(Pc, g, nvalues);
                        T.insert(T.end(), copy.begin(), copy.end());
                        planted.push_back(T.size() - 1);
                        for (unsigned f = rnd(6); f > 0; --f) T.push_back(static_cast<uint8_t>(rnd(nvalues)));
                    }
                    while (T.size() < off + 40 || T.size() % 32 == 0) T.push_back(static_cast<uint8_t>(rnd(nvalues)));
                    const Planes text(T, planes);
                    bool ok = true;
                    // ends clipped at the range's start: 1 column, fewer than m, fewer than m + k, then the first unclipped
                    // ones; at k = 7 on four values EVERY number of columns from 1 to m + k
                    const bool every = k == 7 && nvalues == 4 && !sets;
                    for (size_t c = 1; c <= size_t(m) + k + 2; ++c) {
                        const bool chosen = c <= 3 || c + 1 == m || c == m || c == m + 1 || c + 1 >= size_t(m) + k;
                        if ((every || chosen) && off + c - 1 < T.size()) ok = end_agrees(q, A, T, text, off, off + c - 1, k, &seen) && ok;
                    }
                    // around every planted copy's end, and the text's last symbol (its dword's upper bits are guard bits)
                    for (size_t e : planted)
                        for (size_t x = e - 1; x <= e + 1 && x < T.size(); ++x) ok = end_agrees(q, A, T, text, off, x, k, &seen) && ok;
                    ok = end_agrees(q, A, T, text, off, T.size() - 1, k, &seen) && ok;
                    // every phase e % 32, at the end of the text
                    for (size_t e = T.size() - 32; e < T.size(); ++e) ok = end_agrees(q, A, T, text, off, e, k, &seen) && ok;
                    // a range that begins at symbol 0, where the windows of e < 288 reach below dword 0 of the planes
                    for (size_t e : {size_t(0), size_t(1), size_t(2), size_t(31), size_t(32), size_t(33), size_t(286), size_t(287), size_t(288), size_t(289)})
                        if (e < T.size()) ok = end_agrees(q, A, T, text, 0, e, k, &seen) && ok;
                    ok = end_agrees(q, A, T, text, 0, planted[0], k, &seen) && ok;
                    check(ok, "starts, distances, operations and packing", m, nvalues + (sets ? 100 : 0), k);
                }
            }
        }
        // (the inputs: both kinds of end, all 32 phases of e % 32, clipped ends, windows below dword 0, every number of columns)
        bool all_cols = true;
        for (unsigned c = 1; c <= m + 7; ++c) all_cols = all_cols && seen.ncols[c];
        check(seen.hits > 0 && seen.misses > 0 && seen.phases == 0xffffffffu && seen.clipped > 0 && seen.below > 0 && all_cols,
              "occurrences, non-occurrences, every phase, clipped ends, small ends and every number of columns were exercised", m, seen.hits, seen.misses,
              seen.phases);
    }
}

}  // namespace

int main()
{
    align_cases();
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
