// packed_edit_check.cpp — the host side of the edit-distance calls on the CPU (tests/test_packed_edit.py builds it with
// AddressSanitizer and UBSan and runs it): the recurrence step of smart_amd/csrc/edit_step.hpp for WORDS = 1 and 2 against
// a scalar column-by-column DP, the fresh starts the kernels rely on, and the masks of pedit_host.hpp.
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
#include "edit_step.hpp"
#include "pedit_host.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace {

int g_cases = 0, g_failures = 0;

void check(bool ok, const char* what, unsigned a = 0, unsigned b = 0, unsigned c = 0)
{
    ++g_cases;
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s (%u, %u, %u)\n", what, a, b, c);
}

unsigned long long g_x = 88172645463325252ull;
unsigned rnd(unsigned mod)
{
    g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17;
    return static_cast<unsigned>((g_x >> 11) % mod);
}

// accept[j] bit c: pattern position j accepts code c.  The last row of Sellers' DP over codes[from, to): D[0][*] = 0, the
// column before `from` is D[i] = i.  out[e - from] = D[m][e].
std::vector<int> dp_scores(const std::vector<uint8_t>& accept, const std::vector<uint8_t>& codes, size_t from, size_t to)
{
    const size_t m = accept.size();
    std::vector<int> col(m + 1), next(m + 1), out;
    for (size_t i = 0; i <= m; ++i) col[i] = static_cast<int>(i);
    for (size_t e = from; e < to; ++e) {
        next[0] = 0;
        for (size_t i = 1; i <= m; ++i) {
            const int sub = col[i - 1] + ((accept[i - 1] >> codes[e] & 1) ? 0 : 1);
            next[i] = std::min(sub, std::min(col[i] + 1, next[i - 1] + 1));
        }
        col.swap(next);
        out.push_back(col[m]);
    }
    return out;
}

// the same row by edit_step from a fresh column
template <int WORDS>
std::vector<int> step_scores(const uint32_t (&peq)[4][sg::kEditWords], uint32_t m, const std::vector<uint8_t>& codes, size_t from, size_t to)
{
    uint32_t pv[WORDS], mv[WORDS];
    sg::edit_fresh<WORDS>(pv, mv);
    int score = static_cast<int>(m);
    std::vector<int> out;
    for (size_t e = from; e < to; ++e) {
        uint32_t eq[WORDS];
        for (int w = 0; w < WORDS; ++w) eq[w] = peq[codes[e]][w];
        score += sg::edit_step<WORDS>(pv, mv, eq, m - 1);
        out.push_back(score);
    }
    return out;
}

void accept_to_peq(const std::vector<uint8_t>& accept, uint32_t (&peq)[4][sg::kEditWords])
{
    for (auto& row : peq)
        for (auto& w : row) w = 0;
    for (size_t j = 0; j < accept.size(); ++j)
        for (unsigned c = 0; c < 4; ++c)
            if (accept[j] >> c & 1) peq[c][j >> 5] |= 1u << (j & 31);
}

template <int WORDS>
void recurrence_cases()
{
    const unsigned ms[] = {1, 2, 31, 32, 33, 63, 64};
    const size_t n = 300;
    for (unsigned m : ms) {
        if (m > 32u * WORDS) continue;
        for (unsigned nvalues = 1; nvalues <= 4; ++nvalues) {
            // a random text; the pattern cut from it with a few edits, then a pattern of random SETS (some empty, some full)
            std::vector<uint8_t> codes(n);
            for (auto& c : codes) c = static_cast<uint8_t>(rnd(nvalues));
            for (int kind = 0; kind < 2; ++kind) {
                std::vector<uint8_t> accept(m);
                for (unsigned j = 0; j < m; ++j) {
                    if (kind == 0) accept[j] = rnd(8) == 0 ? static_cast<uint8_t>(1u << rnd(nvalues)) : static_cast<uint8_t>(1u << codes[100 + j]);
                    else accept[j] = static_cast<uint8_t>(rnd(1u << nvalues));
                }
                uint32_t peq[4][sg::kEditWords];
                accept_to_peq(accept, peq);
                const std::vector<int> want = dp_scores(accept, codes, 0, n);
                check(step_scores<WORDS>(peq, m, codes, 0, n) == want, "every column's score", WORDS, m, nvalues);
                // fresh starts at e - (m + k): exact wherever the full value is <= k, above k everywhere else
                for (unsigned k : {0u, 1u, 3u, 7u}) {
                    bool ok = true;
                    for (size_t e = 0; e < n; ++e) {
                        const size_t from = e > m + k ? e - (m + k) : 0;
                        const int got = step_scores<WORDS>(peq, m, codes, from, e + 1).back();
                        ok = ok && (want[e] <= static_cast<int>(k) ? got == want[e] : got > static_cast<int>(k));
                    }
                    check(ok, "fresh start at e - (m + k)", WORDS, m, k);
                }
            }
        }
        // the all-equal pattern on an all-equal text: the addition's carry runs through every bit
        {
            std::vector<uint8_t> codes(n, 1), accept(m, 2);
            uint32_t peq[4][sg::kEditWords];
            accept_to_peq(accept, peq);
            const std::vector<int> got = step_scores<WORDS>(peq, m, codes, 0, n), want = dp_scores(accept, codes, 0, n);
            check(got == want && got[n - 1] == 0 && got[0] == static_cast<int>(m) - 1, "all-equal pattern and text", WORDS, m);
        }
    }
}

void peq_cases()
{
    for (int nvalues = 1; nvalues <= 4; ++nvalues) {
        const uint8_t values[4] = {'A', 'C', 'G', 'T'};
        for (unsigned m : {1u, 31u, 32u, 33u, 64u}) {
            // byte patterns: a held byte has its bit in its code's mask alone, a foreign byte ('N', or a value beyond nvalues) in none
            std::vector<uint8_t> P(m);
            for (unsigned j = 0; j < m; ++j) P[j] = j % 5 == 4 ? 'N' : values[rnd(4)];
            uint32_t peq[4][sg::kEditWords];
            sg::edit_peq_pattern(values, nvalues, P.data(), m, peq);
            bool ok = true;
            for (unsigned j = 0; j < 32 * sg::kEditWords; ++j)
                for (int c = 0; c < 4; ++c) {
                    const bool bit = peq[c][j >> 5] >> (j & 31) & 1;
                    ok = ok && bit == (j < m && c < nvalues && P[j] == values[c]);
                }
            check(ok, "edit_peq_pattern", nvalues, m);
            // sets: empty sets get no bit, a full set a bit in every held code's mask, nothing beyond m
            std::vector<uint8_t> sets(m);
            const unsigned all = (1u << nvalues) - 1u;
            for (unsigned j = 0; j < m; ++j) sets[j] = j % 4 == 0 ? 0 : j % 4 == 1 ? static_cast<uint8_t>(all) : static_cast<uint8_t>(rnd(all + 1));
            check(sg::edit_peq_sets(nvalues, sets.data(), m, peq) == -1, "edit_peq_sets accepts", nvalues, m);
            ok = true;
            for (unsigned j = 0; j < 32 * sg::kEditWords; ++j)
                for (int c = 0; c < 4; ++c) {
                    const bool bit = peq[c][j >> 5] >> (j & 31) & 1;
                    ok = ok && bit == (j < m && (sets[j] >> c & 1));
                }
            check(ok, "edit_peq_sets", nvalues, m);
            // a bit at or above nvalues: refused, the first such position named
            const unsigned bad = m / 2;
            sets[bad] = static_cast<uint8_t>(1u << nvalues);
            if (bad + 1 < m) sets[m - 1] = 0x80;
            check(sg::edit_peq_sets(nvalues, sets.data(), m, peq) == static_cast<int>(bad), "edit_peq_sets names the bad position", nvalues, m);
        }
    }
}

}  // namespace

int main()
{
    recurrence_cases<1>();
    recurrence_cases<2>();
    peq_cases();
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
