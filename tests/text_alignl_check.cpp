// text_alignl_check.cpp — starts and alignments of LONG edit-distance occurrences on byte texts on the CPU
// (tests/test_text_alignl.py builds it with AddressSanitizer and UBSan and runs it): smart_amd/csrc/alignl_band.hpp run as
// text_editl_align (k_talignl.hip) runs it — 64 lanes, one per diagonal, stepped over the anti-diagonals with each lane's
// neighbours taken from the previous step's values; the word-major table of the REVERSED pattern (teditl_host.hpp); every
// byte taken by shift from the wave's window of 73 aligned dwords that ends with dword e >> 2; min(m + k, e - off + 1)
// columns; decisions packed sixteen rows per dword as [row / 16][lane]; the key reduction; the wave-uniform walk with lane
// t / 32 holding word t / 32 — against a scalar full-matrix DP of the suffix distances written out here in forward
// coordinates: the definition of smartgpu_align_editl64 (include/smartgpu.h).
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
#include "alignl_band.hpp"
#include "teditl_host.hpp"

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

// The text as the device holds it, in whole dwords with a front pad below byte 0 and a few bytes behind the last.  The
// device's pad is zero; this one is RANDOM, so a band that consumed a byte of it would disagree with the definition.
constexpr size_t kPad = 4 * sg::kAlignlWinDw;
struct Text {
    std::vector<uint32_t> store;
    size_t n;
    explicit Text(const std::vector<uint8_t>& bytes) : store((kPad + bytes.size() + 7) / 4), n(bytes.size())
    {
        uint8_t* p = reinterpret_cast<uint8_t*>(store.data());
        for (size_t i = 0; i < kPad; ++i) p[i] = static_cast<uint8_t>(rnd(256));
        std::memcpy(p + kPad, bytes.data(), n);
    }
    uint32_t dword(long long x) const { return store.at(static_cast<size_t>(static_cast<long long>(kPad / 4) + x)); }  // text dword x, x >= -kPad / 4
};

struct Result {
    bool hit = false;      // D(e) <= k
    size_t start = 0;
    int dist = 0;
    std::vector<uint8_t> ops;
    bool operator==(const Result& o) const { return hit == o.hit && (!hit || (start == o.start && dist == o.dist && ops == o.ops)); }
};

// ---- the definition: S[i][p] = ed(P[i..m), T[p..e]) for lo <= p <= e + 1, lo = max(off, e + 1 - (m + k)) ----
Result scalar_align(const std::vector<uint8_t>& P, const std::vector<uint8_t>& T, size_t off, size_t e, unsigned k)
{
    const size_t m = P.size();
    const size_t lo = e + 1 - off > m + k ? e + 1 - (m + k) : off;
    const size_t W = e + 1 - lo;  // bytes lo .. e; column index c = p - lo, 0 .. W (W: the empty suffix)
    std::vector<std::vector<int>> S(m + 1, std::vector<int>(W + 1));
    for (size_t c = 0; c <= W; ++c) S[m][c] = static_cast<int>(W - c);
    for (size_t i = m; i-- > 0;) {
        S[i][W] = static_cast<int>(m - i);
        for (size_t c = W; c-- > 0;) {
            const int sub = S[i + 1][c + 1] + (P[i] == T[lo + c] ? 0 : 1);
            S[i][c] = std::min(sub, std::min(S[i + 1][c] + 1, S[i][c + 1] + 1));
        }
    }
    Result r;
    size_t best = W;  // the LARGEST start among the minimisers
    for (size_t c = W; c-- > 0;)
        if (S[0][c] < S[0][best]) best = c;
    r.dist = S[0][best];
    r.hit = r.dist <= static_cast<int>(k);
    r.start = lo + best;
    if (!r.hit) return r;
    size_t i = 0, c = best;
    while (i < m || c < W) {
        if (i < m && c < W) {
            const bool acc = P[i] == T[lo + c];
            if (S[i + 1][c + 1] + (acc ? 0 : 1) == S[i][c]) {
                r.ops.push_back(acc ? 0 : 1);
                ++i; ++c;
                continue;
            }
        }
        if (i < m && S[i + 1][c] + 1 == S[i][c]) {
            r.ops.push_back(3);
            ++i;
        } else {
            r.ops.push_back(2);
            ++c;
        }
    }
    return r;
}

// The kernel's table: editl_peq_bytes of the reversed bytes, word-major, 2, 4 or 8 dwords per byte value
std::vector<uint32_t> reversed_table(const std::vector<uint8_t>& P, uint32_t words)
{
    const uint32_t m = static_cast<uint32_t>(P.size());
    static uint32_t peq[256][sg::kTEditlWords];
    std::vector<uint8_t> rev(m);
    sg::talign_reverse_bytes(P.data(), m, rev.data());
    sg::editl_peq_bytes(rev.data(), m, peq);
    std::vector<uint32_t> table(256u * words);
    sg::editl_peq_table(peq, words, table.data());
    return table;
}

// ---- the same through alignl_band.hpp, as the wave runs it ----
Result band_align(const std::vector<uint32_t>& table, uint32_t m, const Text& text, size_t off, size_t e, unsigned k, bool* packing_ok)
{
    constexpr uint32_t kLanes = sg::kAlignlLanes, kDw = sg::kAlignlWinDw;
    uint32_t win[kDw];
    const long long first = sg::talign_window_first(e, kDw);
    for (uint32_t w = 0; w < kDw; ++w) win[w] = text.dword(first + w);
    if (first + kDw - 1 != static_cast<long long>(e >> 2)) *packing_ok = false;  // nothing above dword e >> 2
    const uint32_t ncols = sg::talign_columns(e, off, m + k);

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
                const uint32_t wb = sg::talign_window_byte(e, j, kDw);
                const uint32_t byte = (win[wb >> 2] >> (8u * (wb & 3u))) & 255u;
                const uint32_t miss = sg::alignl_miss(i, table.at(sg::alignl_peq_index(i, byte)));
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
    unsigned hits = 0, misses = 0, phases = 0, empty = 0, clipped = 0;  // phases: bit e % 4; empty: a hit with J = 0
};

bool end_agrees(const std::vector<uint32_t>& table, const std::vector<uint8_t>& P, const std::vector<uint8_t>& T, const Text& text, size_t off, size_t e,
                unsigned k, Seen* seen)
{
    bool packing = true;
    const Result want = scalar_align(P, T, off, e, k);
    const Result got = band_align(table, static_cast<uint32_t>(P.size()), text, off, e, k, &packing);
    ++(want.hit ? seen->hits : seen->misses);
    seen->phases |= 1u << (e & 3);
    if (want.hit && want.start == e + 1) ++seen->empty;
    if (e - off + 1 < P.size() + k) ++seen->clipped;
    if (!(want == got) || !packing)
        std::printf("  e = %zu off = %zu: want hit %d start %zu dist %d L %zu, got hit %d start %zu dist %d L %zu, packing %d\n", e, off, (int)want.hit,
                    want.start, want.dist, want.ops.size(), (int)got.hit, got.start, got.dist, got.ops.size(), (int)packing);
    return want == got && packing;
}

std::vector<uint8_t> alphabet(unsigned nvalues)
{
    if (nvalues == 1) return {'a'};
    if (nvalues == 2) return {0, 255};
    if (nvalues == 4) return {'A', 'C', 'G', 'T'};
    std::vector<uint8_t> all(256);
    for (unsigned v = 0; v < 256; ++v) all[v] = static_cast<uint8_t>(v);
    return all;
}

// a copy of P with g edits of mixed kinds at random places
std::vector<uint8_t> edited(const std::vector<uint8_t>& P, unsigned g, const std::vector<uint8_t>& vals)
{
    std::vector<uint8_t> c = P;
    for (unsigned x = 0; x < g; ++x) {
        const unsigned kind = rnd(3);
        const uint8_t v = vals[rnd(static_cast<unsigned>(vals.size()))];
        if (kind == 0 && !c.empty()) c[rnd(static_cast<unsigned>(c.size()))] = v;
        else if (kind == 1) c.insert(c.begin() + rnd(static_cast<unsigned>(c.size()) + 1), v);
        else if (!c.empty()) c.erase(c.begin() + rnd(static_cast<unsigned>(c.size())));
    }
    return c;
}

void align_cases()
{
    const unsigned ms[] = {1, 2, 31, 32, 33, 64, 65, 128, 129, 255, 256};
    const size_t off = 37;  // a range that starts inside the text, mid-dword
    for (unsigned m : ms) {
        Seen seen;
        const uint32_t words = m <= 64 ? 2u : m <= 128 ? 4u : 8u;
        for (unsigned nvalues : {1u, 2u, 4u, 256u}) {
            const std::vector<uint8_t> vals = alphabet(nvalues);
            std::vector<uint8_t> P(m);
            for (auto& c : P) c = vals[rnd(nvalues)];
            const std::vector<uint32_t> table = reversed_table(P, words);
            for (unsigned k : {0u, 1u, 7u, 8u, 31u}) {  // (k >= m at m = 1, 2 and, for k = 31, at m = 31: J = 0 is possible)
                // the text: filler, then planted copies with 0 .. k + 1 mixed edits, a few filler bytes between them
                std::vector<uint8_t> T(off + 3);
                for (auto& c : T) c = vals[rnd(nvalues)];
                std::vector<size_t> planted;
                for (unsigned g = 0; g <= k + 1; ++g) {
                    const std::vector<uint8_t> copy = edited(P, g, vals);
                    T.insert(T.end(), copy.begin(), copy.end());
                    planted.push_back(T.size() - 1);
                    for (unsigned f = rnd(6); f > 0; --f) T.push_back(vals[rnd(nvalues)]);
                }
                T.push_back(vals[rnd(nvalues)]);
                const Text text(T);
                bool ok = true;
                // ends clipped at the range's start: 1 column, fewer than m, fewer than m + k; then the first unclipped ones
                for (size_t c : {size_t(1), size_t(2), size_t(3), size_t(m) - 1, size_t(m), size_t(m) + 1, size_t(m) + k - 1, size_t(m) + k, size_t(m) + k + 1, size_t(m) + k + 2})
                    if (c >= 1 && off + c - 1 < T.size()) ok = end_agrees(table, P, T, text, off, off + c - 1, k, &seen) && ok;
                // around every planted copy's end, and the text's last byte; the same ends in a range that begins at byte 0,
                // where the first windows reach below it
                for (size_t e : planted)
                    for (size_t x = e - 1; x <= e + 1 && x < T.size(); ++x) ok = end_agrees(table, P, T, text, off, x, k, &seen) && ok;
                ok = end_agrees(table, P, T, text, off, T.size() - 1, k, &seen) && ok;
                for (size_t e = 0; e < 6 && e < T.size(); ++e) ok = end_agrees(table, P, T, text, 0, e, k, &seen) && ok;
                ok = end_agrees(table, P, T, text, 0, planted[0], k, &seen) && ok;
                check(ok, "starts, distances, operations and packing", m, nvalues, k);
            }
        }
        // (the inputs: both kinds of end, all four phases of e % 4 and clipped ends were seen at this length; the empty match where m <= 2)
        check(seen.hits > 0 && seen.misses > 0 && seen.phases == 15u && seen.clipped > 0 && (m > 2 || seen.empty > 0),
              "occurrences, non-occurrences, every phase, clipped ends and the empty match were exercised", m, seen.hits, seen.misses, seen.empty);
    }
}

// the cell rule by itself: the value is the minimum, the operation the first that applies of diagonal, 'D', 'I'
void cell_cases()
{
    bool ok = true;
    for (int diag = 0; diag < 4; ++diag)
        for (int up = 0; up < 4; ++up)
            for (int left = 0; left < 4; ++left)
                for (uint32_t miss = 0; miss < 2; ++miss) {
                    const sg::AlignlCell c = sg::alignl_cell(diag, up, left, miss);
                    const int v = std::min(diag + (int)miss, std::min(up + 1, left + 1));
                    const uint32_t op = diag + (int)miss == v ? (miss ? sg::kOpSub : sg::kOpEq) : up + 1 == v ? sg::kOpDel : sg::kOpIns;
                    ok = ok && c.value == v && c.op == op;
                }
    check(ok, "the cell rule");
}

}  // namespace

int main()
{
    cell_cases();
    align_cases();
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
