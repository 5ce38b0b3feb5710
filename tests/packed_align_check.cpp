// packed_align_check.cpp — starts and alignments of edit-distance occurrences on the CPU (tests/test_packed_align.py builds
// it with AddressSanitizer and UBSan and runs it): the distance-form step, the cell values and the traceback of
// smart_amd/csrc/edit_align.hpp, fed as planes_edit_align feeds them (the masks of the REVERSED pattern, the text backward
// from e, min(m + k, e - off + 1) columns), against a scalar DP of the suffix distances written out here in forward
// coordinates — the definition of smartgpu_palign_edit64 (include/smartgpu.h).
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
#include "edit_align.hpp"
#include "pedit_host.hpp"

#include <algorithm>
#include <cstdio>
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

struct Result {
    bool hit = false;      // D(e) <= k
    size_t start = 0;
    int dist = 0;
    std::vector<uint8_t> ops;
    bool operator==(const Result& o) const { return hit == o.hit && (!hit || (start == o.start && dist == o.dist && ops == o.ops)); }
};

// ---- the definition: S[i][p] = ed(P[i..m), T[p..e]) for lo <= p <= e + 1, lo = max(off, e + 1 - (m + k)) ----
Result scalar_align(const std::vector<uint8_t>& accept, const std::vector<uint8_t>& codes, size_t off, size_t e, unsigned k)
{
    const size_t m = accept.size();
    const size_t lo = e + 1 - off > m + k ? e + 1 - (m + k) : off;
    const size_t W = e + 1 - lo;  // symbols lo .. e; column index c = p - lo, 0 .. W (W: the empty suffix)
    std::vector<std::vector<int>> S(m + 1, std::vector<int>(W + 1));
    for (size_t c = 0; c <= W; ++c) S[m][c] = static_cast<int>(W - c);
    for (size_t i = m; i-- > 0;) {
        S[i][W] = static_cast<int>(m - i);
        for (size_t c = W; c-- > 0;) {
            const int sub = S[i + 1][c + 1] + ((accept[i] >> codes[lo + c] & 1) ? 0 : 1);
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
            const bool acc = accept[i] >> codes[lo + c] & 1;
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

// ---- the same through edit_align.hpp, as the kernel runs it ----
template <int WORDS>
Result vector_align(const std::vector<uint8_t>& accept, const std::vector<uint8_t>& codes, size_t off, size_t e, unsigned k, bool* packing_ok)
{
    const uint32_t m = static_cast<uint32_t>(accept.size());
    uint32_t peq[4][sg::kEditWords] = {};
    for (uint32_t j = 0; j < m; ++j)  // the REVERSED pattern
        for (unsigned c = 0; c < 4; ++c)
            if (accept[m - 1 - j] >> c & 1) peq[c][j >> 5] |= 1u << (j & 31);
    const uint32_t ncols = static_cast<uint32_t>(std::min<size_t>(m + k, e - off + 1));
    std::vector<uint32_t> cpv(static_cast<size_t>(ncols) * WORDS), cmv(static_cast<size_t>(ncols) * WORDS);
    uint32_t pv[WORDS], mv[WORDS];
    sg::edit_fresh<WORDS>(pv, mv);
    int score = static_cast<int>(m), best = score;
    uint32_t J = 0;
    for (uint32_t j = 1; j <= ncols; ++j) {
        uint32_t eq[WORDS];
        for (int w = 0; w < WORDS; ++w) eq[w] = peq[codes[e - (j - 1)]][w];
        score += sg::edit_step_dist<WORDS>(pv, mv, eq, m - 1);
        for (int w = 0; w < WORDS; ++w) {
            cpv[(j - 1) * WORDS + w] = pv[w];
            cmv[(j - 1) * WORDS + w] = mv[w];
        }
        // every cell of the column's last row agrees with the running score
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
        for (int w = 0; w < WORDS; ++w) {
            opv[w] = j ? cpv[(j - 1) * WORDS + w] : ~0u;
            omv[w] = j ? cmv[(j - 1) * WORDS + w] : 0u;
            oeq[w] = j ? peq[codes[e - (j - 1)]][w] : 0u;
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

// every listed end of the range [off, n): start, distance and operations equal the definition's; a non-occurrence on both sides
template <int WORDS>
bool ends_agree(const std::vector<uint8_t>& accept, const std::vector<uint8_t>& codes, size_t off, size_t e_first, size_t e_last, unsigned k,
                unsigned* hits, unsigned* misses)
{
    bool ok = true, packing = true;
    for (size_t e = e_first; e <= e_last; ++e) {
        const Result want = scalar_align(accept, codes, off, e, k), got = vector_align<WORDS>(accept, codes, off, e, k, &packing);
        ok = ok && want == got;
        ++*(want.hit ? hits : misses);
    }
    return ok && packing;
}

template <int WORDS>
void align_cases()
{
    const unsigned ms[] = {1, 2, 31, 32, 33, 63, 64};
    const size_t n = 200;
    for (unsigned m : ms) {
        if (m > 32u * WORDS) continue;
        unsigned hits = 0, misses = 0;
        for (unsigned nvalues = 1; nvalues <= 4; ++nvalues) {
            std::vector<uint8_t> codes(n);
            for (auto& c : codes) c = static_cast<uint8_t>(rnd(nvalues));
            for (int kind = 0; kind < 2; ++kind) {
                // a byte pattern cut from the text with a few symbols changed, then a pattern of random SETS (some empty, some full)
                std::vector<uint8_t> accept(m);
                for (unsigned j = 0; j < m; ++j) {
                    if (kind == 0) accept[j] = rnd(8) == 0 ? static_cast<uint8_t>(1u << rnd(nvalues)) : static_cast<uint8_t>(1u << codes[100 + j]);
                    else accept[j] = static_cast<uint8_t>(rnd(1u << nvalues));
                }
                for (unsigned k : {0u, 1u, 3u, 7u}) {
                    // every end of the whole text: the first m + k - 1 walks are clipped at symbol 0, down to ONE column at e = 0
                    check(ends_agree<WORDS>(accept, codes, 0, 0, n - 1, k, &hits, &misses), "every end of the text", WORDS, m, nvalues, k);
                    // a range that starts inside the text, at a position that is no multiple of 32: ends off .. off + m + k
                    const size_t off = 37;
                    check(ends_agree<WORDS>(accept, codes, off, off, off + m + k, k, &hits, &misses), "walks clipped at off", WORDS, m, nvalues, k);
                }
            }
        }
        // (the inputs: both kinds of end were seen at this length)
        check(hits > 0 && misses > 0, "occurrences and non-occurrences were both exercised", WORDS, m, hits, misses);
        // the all-equal pattern on an all-equal text: the addition's carry runs through every bit; every end from m - 1 on is
        // exact, its start e - m + 1 and its operations m times '='
        {
            std::vector<uint8_t> codes(n, 1), accept(m, 2);
            bool ok = true, packing = true;
            for (unsigned k : {0u, 1u, 3u, 7u})
                for (size_t e = 0; e < n; ++e) {
                    const Result want = scalar_align(accept, codes, 0, e, k), got = vector_align<WORDS>(accept, codes, 0, e, k, &packing);
                    ok = ok && want == got;
                    if (e + 1 >= m) ok = ok && got.hit && got.dist == 0 && got.start == e + 1 - m && got.ops == std::vector<uint8_t>(m, 0);
                }
            check(ok && packing, "all-equal pattern and text", WORDS, m);
        }
        // a pattern that accepts nothing: D(e) = m at every end — above k = 0, so no end is an occurrence
        {
            std::vector<uint8_t> codes(n), accept(m, 0);
            for (auto& c : codes) c = static_cast<uint8_t>(rnd(4));
            bool ok = true, packing = true;
            for (size_t e = 0; e < n; ++e) {
                const Result want = scalar_align(accept, codes, 0, e, 0), got = vector_align<WORDS>(accept, codes, 0, e, 0, &packing);
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
