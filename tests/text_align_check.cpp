// text_align_check.cpp — starts and alignments of edit-distance occurrences on BYTE texts on the CPU (tests/test_text_align.py
// builds it with AddressSanitizer and UBSan and runs it): smart_amd/csrc/talign_host.hpp and edit_align.hpp fed as
// text_edit_align (k_talign.hip) feeds them — the 256-mask table of the REVERSED pattern (bytes or class rows), every byte
// taken by shift from the lane's window of aligned dwords that ends with dword e >> 2, min(m + k, e - off + 1) columns —
// against a scalar DP of the suffix distances written out here in forward coordinates: the definition of
// smartgpu_align_edit64 (include/smartgpu.h).
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
#include "edit_align.hpp"
#include "talign_host.hpp"

#include <algorithm>
#include <array>
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

using Row = std::array<uint8_t, 32>;  // a class: bit v % 8 of byte v / 8 = the position accepts byte v
bool accepts(const Row& r, uint8_t v) { return r[v >> 3] >> (v & 7) & 1; }
Row singleton(uint8_t v)
{
    Row r{};
    r[v >> 3] = static_cast<uint8_t>(1u << (v & 7));
    return r;
}

// The text as the device holds it, in whole dwords with a front pad below byte 0 and a few bytes behind the last.  The
// device's pad is zero; this one is RANDOM, so a walk that consumed a byte of it would disagree with the definition.
constexpr size_t kPad = 128;
struct Text {
    std::vector<uint32_t> store;
    size_t n;
    explicit Text(const std::vector<uint8_t>& bytes) : store((kPad + bytes.size() + 7) / 4), n(bytes.size())
    {
        uint8_t* p = reinterpret_cast<uint8_t*>(store.data());
        for (size_t i = 0; i < kPad; ++i) p[i] = static_cast<uint8_t>(rnd(256));
        std::memcpy(p + kPad, bytes.data(), n);
    }
    uint32_t dword(long long x) const { return store[static_cast<size_t>(static_cast<long long>(kPad / 4) + x)]; }  // text dword x, x >= -kPad / 4
};

struct Result {
    bool hit = false;      // D(e) <= k
    size_t start = 0;
    int dist = 0;
    std::vector<uint8_t> ops;
    bool operator==(const Result& o) const { return hit == o.hit && (!hit || (start == o.start && dist == o.dist && ops == o.ops)); }
};

// ---- the definition: S[i][p] = ed(P[i..m), T[p..e]) for lo <= p <= e + 1, lo = max(off, e + 1 - (m + k)) ----
Result scalar_align(const std::vector<Row>& pat, const std::vector<uint8_t>& T, size_t off, size_t e, unsigned k)
{
    const size_t m = pat.size();
    const size_t lo = e + 1 - off > m + k ? e + 1 - (m + k) : off;
    const size_t W = e + 1 - lo;  // bytes lo .. e; column index c = p - lo, 0 .. W (W: the empty suffix)
    std::vector<std::vector<int>> S(m + 1, std::vector<int>(W + 1));
    for (size_t c = 0; c <= W; ++c) S[m][c] = static_cast<int>(W - c);
    for (size_t i = m; i-- > 0;) {
        S[i][W] = static_cast<int>(m - i);
        for (size_t c = W; c-- > 0;) {
            const int sub = S[i + 1][c + 1] + (accepts(pat[i], T[lo + c]) ? 0 : 1);
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
            const bool acc = accepts(pat[i], T[lo + c]);
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

// The kernel's table: edit_peq_bytes of the reversed bytes (a pattern of singletons given as bytes), or edit_peq_classes of
// the reversed rows
template <int WORDS>
std::vector<uint32_t> reversed_table(const std::vector<Row>& pat, const std::vector<uint8_t>* bytes)
{
    const uint32_t m = static_cast<uint32_t>(pat.size());
    uint32_t peq[256][sg::kTEditWords];
    if (bytes) {
        std::vector<uint8_t> rev(m);
        sg::talign_reverse_bytes(bytes->data(), m, rev.data());
        sg::edit_peq_bytes(rev.data(), m, peq);
    } else {
        std::vector<uint8_t> flat(32u * m), rev(32u * m);
        for (uint32_t j = 0; j < m; ++j) std::memcpy(flat.data() + 32u * j, pat[j].data(), 32);
        sg::talign_reverse_classes(flat.data(), m, rev.data());
        sg::edit_peq_classes(rev.data(), m, peq);
    }
    std::vector<uint32_t> table(256u * WORDS);
    sg::edit_peq_table(peq, WORDS, table.data());
    return table;
}

// ---- the same through talign_host.hpp and edit_align.hpp, as the kernel runs it ----
template <int WORDS>
Result vector_align(const std::vector<uint32_t>& table, uint32_t m, const Text& text, size_t off, size_t e, unsigned k, bool* packing_ok)
{
    constexpr uint32_t kDw = sg::talign_window_dwords(WORDS);
    static_assert(kDw == (WORDS == 2 ? 19 : 11), "the window of the longest walk");
    uint32_t win[kDw];
    const long long first = sg::talign_window_first(e, kDw);
    for (uint32_t w = 0; w < kDw; ++w) win[w] = text.dword(first + w);
    if (first + kDw - 1 != static_cast<long long>(e >> 2)) *packing_ok = false;  // nothing above dword e >> 2
    const auto eq_of = [&](uint32_t j, uint32_t (&eq)[WORDS]) {
        const uint32_t wb = sg::talign_window_byte(e, j, kDw);
        const uint32_t byte = (win[wb >> 2] >> (8u * (wb & 3u))) & 255u;
        for (int w = 0; w < WORDS; ++w) eq[w] = table[byte * WORDS + w];
    };
    const uint32_t ncols = sg::talign_columns(e, off, m + k);
    std::vector<uint32_t> cpv(static_cast<size_t>(ncols) * WORDS), cmv(static_cast<size_t>(ncols) * WORDS);
    uint32_t pv[WORDS], mv[WORDS];
    sg::edit_fresh<WORDS>(pv, mv);
    int score = static_cast<int>(m), best = score;
    uint32_t J = 0;
    for (uint32_t j = 1; j <= ncols; ++j) {
        uint32_t eq[WORDS];
        eq_of(j, eq);
        score += sg::edit_step_dist<WORDS>(pv, mv, eq, m - 1);
        for (int w = 0; w < WORDS; ++w) {
            cpv[(j - 1) * WORDS + w] = pv[w];
            cmv[(j - 1) * WORDS + w] = mv[w];
        }
        if (sg::edit_cell<WORDS>(pv, mv, m, j) != score) *packing_ok = false;
        if (score < best) {
            best = score;
            J = j;
        }
    }
    Result r;
    r.dist = best;
    r.hit = best <= static_cast<int>(k);
    r.start = e + 1 - J;
    if (!r.hit) return r;
    auto col = [&](uint32_t j, uint32_t (&opv)[WORDS], uint32_t (&omv)[WORDS], uint32_t (&oeq)[WORDS]) {
        const uint32_t row = j ? j - 1 : 0;
        eq_of(row + 1, oeq);
        for (int w = 0; w < WORDS; ++w) {
            opv[w] = j ? cpv[row * WORDS + w] : ~0u;
            omv[w] = j ? cmv[row * WORDS + w] : 0u;
        }
    };
    uint64_t ops[3];
    const uint32_t L = sg::edit_traceback<WORDS>(m, J, best, col, ops);
    if ((ops[2] >> 56) != L || L > sg::kAlignMaxOps) *packing_ok = false;
    for (uint32_t t = 0; t < 96; ++t) {
        const uint64_t word = t / 32 == 2 ? ops[2] & 0x00ffffffffffffffull : ops[t / 32];
        const uint8_t op = static_cast<uint8_t>(word >> (2 * (t % 32)) & 3);
        if (t < L) r.ops.push_back(op);
        else if (op) *packing_ok = false;  // every unused bit is 0
    }
    return r;
}

struct Seen {
    unsigned hits = 0, misses = 0, phases = 0;  // phases: bit e % 4
};

// every listed end of the range [off, n): start, distance and operations equal the definition's; a non-occurrence on both sides
template <int WORDS>
bool ends_agree(const std::vector<Row>& pat, const std::vector<uint8_t>* bytes, const std::vector<uint8_t>& T, const Text& text, size_t off,
                size_t e_first, size_t e_last, unsigned k, Seen* seen)
{
    const std::vector<uint32_t> table = reversed_table<WORDS>(pat, bytes);
    bool ok = true, packing = true;
    for (size_t e = e_first; e <= e_last; ++e) {
        const Result want = scalar_align(pat, T, off, e, k);
        const Result got = vector_align<WORDS>(table, static_cast<uint32_t>(pat.size()), text, off, e, k, &packing);
        ok = ok && want == got;
        ++(want.hit ? seen->hits : seen->misses);
        seen->phases |= 1u << (e & 3);
    }
    return ok && packing;
}

std::vector<uint8_t> alphabet(unsigned nvalues)
{
    if (nvalues == 2) return {0, 255};
    if (nvalues == 4) return {'A', 'C', 'G', 'T'};
    if (nvalues == 20) { const char* a = "ACDEFGHIKLMNPQRSTVWY"; return std::vector<uint8_t>(a, a + 20); }
    std::vector<uint8_t> all(256);
    for (unsigned v = 0; v < 256; ++v) all[v] = static_cast<uint8_t>(v);
    return all;
}

template <int WORDS>
void align_cases()
{
    const unsigned ms[] = {1, 2, 31, 32, 33, 63, 64};
    const size_t n = 200;
    for (unsigned m : ms) {
        if (m > 32u * WORDS) continue;
        Seen seen;
        for (unsigned nvalues : {2u, 4u, 20u, 256u}) {
            const std::vector<uint8_t> vals = alphabet(nvalues);
            std::vector<uint8_t> T(n);
            for (auto& c : T) c = vals[rnd(nvalues)];
            const Text text(T);
            for (int kind = 0; kind < 2; ++kind) {
                // a byte pattern cut from the text with a few bytes changed, then a pattern of random CLASSES with a full row
                // in its middle and, from three positions on, an empty first row
                std::vector<Row> pat(m);
                std::vector<uint8_t> bytes(m);
                for (unsigned j = 0; j < m; ++j) {
                    if (kind == 0) {
                        bytes[j] = rnd(8) == 0 ? vals[rnd(nvalues)] : T[100 + j];
                        pat[j] = singleton(bytes[j]);
                    } else {
                        pat[j] = singleton(T[100 + j]);
                        for (unsigned extra = rnd(4); extra > 0; --extra) {
                            const uint8_t v = vals[rnd(nvalues)];
                            pat[j][v >> 3] |= static_cast<uint8_t>(1u << (v & 7));
                        }
                        if (rnd(6) == 0) pat[j] = Row{};
                    }
                }
                if (kind == 1) {
                    pat[m / 2].fill(255);
                    if (m >= 3) pat[0] = Row{};
                }
                for (unsigned k : {0u, 1u, 3u, 7u}) {
                    // every end of the whole text: the first m + k - 1 walks are clipped at byte 0 — their windows reach below
                    // it —, down to ONE column at e = 0; every e % 4
                    check(ends_agree<WORDS>(pat, kind ? nullptr : &bytes, T, text, 0, 0, n - 1, k, &seen), "every end of the text", WORDS, m, nvalues, k);
                    // a range that starts inside the text, mid-dword: ends off .. off + m + k
                    const size_t off = 37;
                    check(ends_agree<WORDS>(pat, kind ? nullptr : &bytes, T, text, off, off, off + m + k, k, &seen), "walks clipped at off", WORDS, m, nvalues, k);
                }
            }
        }
        // (the inputs: both kinds of end and all four phases of e % 4 were seen at this length)
        check(seen.hits > 0 && seen.misses > 0 && seen.phases == 15u, "occurrences, non-occurrences and every phase were exercised", WORDS, m, seen.hits, seen.misses);
        // FULL rows on any text: every end from m - 1 on is exact, its start e - m + 1 and its operations m times '='
        {
            std::vector<uint8_t> T(n);
            for (auto& c : T) c = static_cast<uint8_t>(rnd(256));
            const Text text(T);
            Row full;
            full.fill(255);
            const std::vector<Row> pat(m, full);
            const std::vector<uint32_t> table = reversed_table<WORDS>(pat, nullptr);
            bool ok = true, packing = true;
            for (unsigned k : {0u, 1u, 3u, 7u})
                for (size_t e = 0; e < n; ++e) {
                    const Result want = scalar_align(pat, T, 0, e, k), got = vector_align<WORDS>(table, m, text, 0, e, k, &packing);
                    ok = ok && want == got;
                    if (e + 1 >= m) ok = ok && got.hit && got.dist == 0 && got.start == e + 1 - m && got.ops == std::vector<uint8_t>(m, 0);
                }
            check(ok && packing, "full rows", WORDS, m);
        }
        // EMPTY rows accept nothing: D(e) = m at every end — above k = 0, so no end is an occurrence
        {
            std::vector<uint8_t> T(n);
            for (auto& c : T) c = static_cast<uint8_t>(rnd(256));
            const Text text(T);
            const std::vector<Row> pat(m, Row{});
            const std::vector<uint32_t> table = reversed_table<WORDS>(pat, nullptr);
            bool ok = true, packing = true;
            for (size_t e = 0; e < n; ++e) {
                const Result want = scalar_align(pat, T, 0, e, 0), got = vector_align<WORDS>(table, m, text, 0, e, 0, &packing);
                ok = ok && !want.hit && !got.hit && want.dist == static_cast<int>(m);
            }
            check(ok && packing, "an end with D(e) > k", WORDS, m);
        }
    }
}

}  // namespace

int main()
{
    align_cases<1>();
    align_cases<2>();
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
