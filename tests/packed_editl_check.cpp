// packed_editl_check.cpp — the host side of the long-pattern edit-distance calls on the CPU (tests/test_packed_editl.py
// builds it with AddressSanitizer and UBSan and runs it): the block recurrence of smart_amd/csrc/edit_block.hpp against a
// scalar column-by-column DP, every column, with the cut-off and with all blocks; the fresh starts the kernels rely on; the
// form the kernels run, 64 lanes in step with ONE number of active blocks; and the masks of peditl_host.hpp.
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
// With the argument "blocks" it prints instead the mean number of active blocks per column on random texts, per lane and
// for a wave of 64 lanes (tools/editl_probe.py puts the figures beside its timings).
#include "edit_block.hpp"
#include "peditl_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>
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

void accept_to_peq(const std::vector<uint8_t>& accept, uint32_t (&peq)[4][sg::kEditlWords])
{
    std::memset(peq, 0, sizeof peq);
    for (size_t j = 0; j < accept.size(); ++j)
        for (unsigned c = 0; c < 4; ++c)
            if (accept[j] >> c & 1) peq[c][j >> 5] |= 1u << (j & 31);
}

constexpr int kAbove = 1 << 20;  // "not computed": the last block is not active, the value is > k

struct Walk {
    std::vector<int> out;        // per column: bot when every block is active, kAbove otherwise
    unsigned max_b = 0, shrinks = 0;
    unsigned long long blocks = 0;  // active blocks summed over the columns
};

// One lane, the rule of edit_block.hpp as written there (cut) or all blocks of every column.
template <int MAXW>
Walk lane_walk(const uint32_t (&peq)[4][sg::kEditlWords], uint32_t m, uint32_t k, bool cut, const std::vector<uint8_t>& codes, size_t from, size_t to)
{
    const uint32_t W = (m + 31) / 32;
    uint32_t pv[MAXW], mv[MAXW], B = cut ? 1u : W;
    int bot;
    sg::block_fresh<MAXW>(pv, mv, B, m, bot);
    Walk r;
    for (size_t e = from; e < to; ++e) {
        if (cut && B < W && sg::block_wants_grow(bot, k)) sg::block_grow<MAXW>(pv, mv, B, m, bot);
        bot += sg::block_step<MAXW>(pv, mv, [&](int w) { return peq[codes[e]][w]; }, B, m);
        r.max_b = std::max(r.max_b, B);
        if (cut)
            while (B > 1u && sg::block_may_shrink(bot, k, B, m)) {
                sg::block_shrink<MAXW>(pv, mv, B, m, bot);
                ++r.shrinks;
            }
        r.blocks += B;
        r.out.push_back(B == W ? bot : kAbove);
    }
    return r;
}

// The form k_peditl.hip runs: 64 lanes in step, lane l on codes[from + l * stride, + len), ONE B — grown when any lane asks
// for it, shrunk when all agree.  out[l]: the lane's columns.
template <int MAXW>
std::vector<Walk> wave_walk(const uint32_t (&peq)[4][sg::kEditlWords], uint32_t m, uint32_t k, const std::vector<uint8_t>& codes, size_t from,
                            size_t stride, size_t len)
{
    constexpr int L = 64;
    const uint32_t W = (m + 31) / 32;
    uint32_t pv[L][MAXW], mv[L][MAXW], B = 1u;
    int bot[L];
    for (int l = 0; l < L; ++l) sg::block_fresh<MAXW>(pv[l], mv[l], B, m, bot[l]);
    std::vector<Walk> r(L);
    for (size_t t = 0; t < len; ++t) {
        bool any = false;
        for (int l = 0; l < L; ++l) any = any || sg::block_wants_grow(bot[l], k);
        if (B < W && any) {
            uint32_t b = B;
            for (int l = 0; l < L; ++l) {
                b = B;
                sg::block_grow<MAXW>(pv[l], mv[l], b, m, bot[l]);
            }
            B = b;
        }
        for (int l = 0; l < L; ++l) {
            const uint8_t code = codes[from + l * stride + t];
            bot[l] += sg::block_step<MAXW>(pv[l], mv[l], [&](int w) { return peq[code][w]; }, B, m);
        }
        for (;;) {
            bool all = B > 1u;
            for (int l = 0; l < L && all; ++l) all = sg::block_may_shrink(bot[l], k, B, m);
            if (!all) break;
            uint32_t b = B;
            for (int l = 0; l < L; ++l) {
                b = B;
                sg::block_shrink<MAXW>(pv[l], mv[l], b, m, bot[l]);
            }
            B = b;
        }
        for (int l = 0; l < L; ++l) {
            r[l].out.push_back(B == W ? bot[l] : kAbove);
            r[l].blocks += B;
        }
    }
    return r;
}

// exact wherever the true value is <= k, above k everywhere else
bool agrees(const std::vector<int>& got, const std::vector<int>& want, uint32_t k)
{
    if (got.size() != want.size()) return false;
    for (size_t i = 0; i < want.size(); ++i)
        if (want[i] <= static_cast<int>(k) ? got[i] != want[i] : got[i] <= static_cast<int>(k)) return false;
    return true;
}

const unsigned kMs[] = {1, 32, 33, 64, 65, 96, 97, 128, 129, 255, 256};
const unsigned kKs[] = {0, 1, 7, 8, 15, 16, 31};

// the width the launchers of k_peditl.hip choose
template <typename F>
void with_width(unsigned m, F f)
{
    if (m <= 64) f(std::integral_constant<int, 2>());
    else if (m <= 128) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 8>());
}

void recurrence_cases()
{
    const size_t n = 700;
    for (unsigned m : kMs)
        with_width(m, [&](auto width) {
            constexpr int MAXW = decltype(width)::value;
            for (unsigned nvalues = 1; nvalues <= 4; ++nvalues) {
                // a random text; the pattern cut from it with a few substitutions, and a second copy of it planted with mixed
                // edits; then a pattern of random SETS (some empty, some full)
                std::vector<uint8_t> codes(n);
                for (auto& c : codes) c = static_cast<uint8_t>(rnd(nvalues));
                for (int kind = 0; kind < 2; ++kind) {
                    std::vector<uint8_t> accept(m);
                    for (unsigned j = 0; j < m; ++j) {
                        if (kind == 0) accept[j] = rnd(16) == 0 ? static_cast<uint8_t>(1u << rnd(nvalues)) : static_cast<uint8_t>(1u << codes[100 + j]);
                        else accept[j] = static_cast<uint8_t>(rnd(1u << nvalues));
                    }
                    if (kind == 0) {  // the copy: one symbol in 24 dropped, one in 24 doubled
                        size_t at = 400;
                        for (unsigned j = 0; j < m && at + 1 < n; ++j) {
                            const unsigned r = rnd(24);
                            if (r == 0) continue;
                            codes[at++] = codes[100 + j];
                            if (r == 1) codes[at++] = static_cast<uint8_t>(rnd(nvalues));
                        }
                    }
                    uint32_t peq[4][sg::kEditlWords];
                    accept_to_peq(accept, peq);
                    const std::vector<int> want = dp_scores(accept, codes, 0, n);
                    std::vector<std::vector<int>> lane_want;  // lane l of the wave below walks [9 l, 9 l + 120)
                    for (size_t l = 0; l < 64; ++l) lane_want.push_back(dp_scores(accept, codes, 9 * l, 9 * l + 120));
                    for (unsigned k : kKs) {
                        check(lane_walk<MAXW>(peq, m, k, false, codes, 0, n).out == want, "all blocks: every column's score", m, nvalues, k);
                        check(agrees(lane_walk<MAXW>(peq, m, k, true, codes, 0, n).out, want, k), "the cut-off: every column", m, nvalues, k);
                        // fresh starts at e - (m + k), with the cut-off
                        bool ok = true;
                        for (size_t e = rnd(5); e < n; e += 5) {
                            const size_t from = e > m + k ? e - (m + k) : 0;
                            const int got = lane_walk<MAXW>(peq, m, k, true, codes, from, e + 1).out.back();
                            ok = ok && (want[e] <= static_cast<int>(k) ? got == want[e] : got > static_cast<int>(k));
                        }
                        check(ok, "fresh start at e - (m + k)", m, nvalues, k);
                        // 64 lanes, one B, each against the DP on its own stretch
                        const std::vector<Walk> wave = wave_walk<MAXW>(peq, m, k, codes, 0, 9, 120);
                        ok = true;
                        for (size_t l = 0; l < 64; ++l) ok = ok && agrees(wave[l].out, lane_want[l], k);
                        check(ok, "64 lanes with one B", m, nvalues, k);
                    }
                }
            }
            // the all-equal pattern on an all-equal text: the addition's carry crosses every block
            {
                std::vector<uint8_t> codes(n, 1), accept(m, 2);
                uint32_t peq[4][sg::kEditlWords];
                accept_to_peq(accept, peq);
                const std::vector<int> want = dp_scores(accept, codes, 0, n);
                const std::vector<int> all = lane_walk<MAXW>(peq, m, 0, false, codes, 0, n).out;
                check(all == want && all[n - 1] == 0 && all[0] == static_cast<int>(m) - 1 && agrees(lane_walk<MAXW>(peq, m, 0, true, codes, 0, n).out, want, 0) &&
                          agrees(lane_walk<MAXW>(peq, m, 31, true, codes, 0, n).out, want, 31),
                      "all-equal pattern and text", m);
            }
            // planted prefixes of the pattern, each followed by a symbol the next position does not accept: blocks switch on and off
            for (unsigned k : {0u, 7u, 31u}) {
                std::vector<uint8_t> accept(m), codes(4000);
                for (auto& a : accept) a = static_cast<uint8_t>(1u << rnd(4));
                for (auto& c : codes) c = static_cast<uint8_t>(rnd(4));
                size_t at = 300;
                unsigned longest = 0;
                for (unsigned len : {31u, 32u, 33u, 64u, 100u, 200u, m - 1}) {
                    if (len == 0 || len >= m) continue;
                    for (unsigned j = 0; j < len; ++j) codes[at + j] = static_cast<uint8_t>(__builtin_ctz(accept[j]));
                    codes[at + len] = static_cast<uint8_t>((__builtin_ctz(accept[len]) + 1) & 3);
                    at += len + 150;
                    longest = std::max(longest, len);
                }
                uint32_t peq[4][sg::kEditlWords];
                accept_to_peq(accept, peq);
                const std::vector<int> want = dp_scores(accept, codes, 0, codes.size());
                const Walk got = lane_walk<MAXW>(peq, m, k, true, codes, 0, codes.size());
                // a prefix of 32 symbols or more of a pattern of more than one block switches the second block on; at a small k the
                // random text behind it switches it off again (at k = 31 a block of random text stays below k + 32: no claim)
                const bool switched = (m + 31) / 32 < 2 || longest < 32 || (got.max_b >= 2 && (k > 7 || got.shrinks >= 1));
                check(agrees(got.out, want, k) && switched && lane_walk<MAXW>(peq, m, k, false, codes, 0, codes.size()).out == want, "planted prefixes", m, k,
                      got.max_b);
            }
        });
}

void peq_cases()
{
    for (int nvalues = 1; nvalues <= 4; ++nvalues) {
        const uint8_t values[4] = {'A', 'C', 'G', 'T'};
        for (unsigned m : {1u, 33u, 255u, 256u}) {
            std::vector<uint8_t> P(m);
            for (unsigned j = 0; j < m; ++j) P[j] = j % 5 == 4 ? 'N' : values[rnd(4)];
            uint32_t peq[4][sg::kEditlWords];
            sg::editl_peq_pattern(values, nvalues, P.data(), m, peq);
            bool ok = true;
            for (unsigned j = 0; j < 32 * sg::kEditlWords; ++j)
                for (int c = 0; c < 4; ++c) {
                    const bool bit = peq[c][j >> 5] >> (j & 31) & 1;
                    ok = ok && bit == (j < m && c < nvalues && P[j] == values[c]);
                }
            check(ok, "editl_peq_pattern", nvalues, m);
            std::vector<uint8_t> sets(m);
            const unsigned all = (1u << nvalues) - 1u;
            for (unsigned j = 0; j < m; ++j) sets[j] = j % 4 == 0 ? 0 : j % 4 == 1 ? static_cast<uint8_t>(all) : static_cast<uint8_t>(rnd(all + 1));
            ok = sg::editl_peq_sets(nvalues, sets.data(), m, peq) == -1;
            for (unsigned j = 0; j < 32 * sg::kEditlWords; ++j)
                for (int c = 0; c < 4; ++c) {
                    const bool bit = peq[c][j >> 5] >> (j & 31) & 1;
                    ok = ok && bit == (j < m && (sets[j] >> c & 1));
                }
            check(ok, "editl_peq_sets", nvalues, m);
            const unsigned bad = m / 2;
            sets[bad] = static_cast<uint8_t>(1u << nvalues);
            if (bad + 1 < m) sets[m - 1] = 0x80;
            check(sg::editl_peq_sets(nvalues, sets.data(), m, peq) == static_cast<int>(bad), "editl_peq_sets names the bad position", nvalues, m);
        }
    }
}

// mean active blocks per column on random texts: "blocks <text> <m> <k> <per lane> <per wave of 64>"
void block_counts()
{
    const size_t len = 4000, stride = 512;
    for (unsigned nvalues : {4u, 2u}) {
        std::vector<uint8_t> codes(64 * stride + len);
        for (auto& c : codes) c = static_cast<uint8_t>(rnd(nvalues));
        for (unsigned m : {64u, 65u, 100u, 150u, 256u})
            with_width(m, [&](auto width) {
                constexpr int MAXW = decltype(width)::value;
                std::vector<uint8_t> accept(m);
                for (auto& a : accept) a = static_cast<uint8_t>(1u << rnd(nvalues));
                uint32_t peq[4][sg::kEditlWords];
                accept_to_peq(accept, peq);
                for (unsigned k : {0u, 3u, 7u, 15u, 31u}) {
                    const Walk one = lane_walk<MAXW>(peq, m, k, true, codes, 0, codes.size());
                    const std::vector<Walk> wave = wave_walk<MAXW>(peq, m, k, codes, 0, stride, len);
                    std::printf("blocks rand%u %u %u %.3f %.3f\n", nvalues, m, k, static_cast<double>(one.blocks) / codes.size(),
                                static_cast<double>(wave[0].blocks) / len);
                }
            });
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "blocks")) {
        block_counts();
        return 0;
    }
    recurrence_cases();
    peq_cases();
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
