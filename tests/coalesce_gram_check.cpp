// coalesce_gram_check.cpp — the shared skip table of hor_multi_scan (smart_amd/csrc/multi.hpp) on the host: the table built
// serially with the functions the kernel uses, a text walked 64 window ends at a time as a lane walks its segment, every
// pattern's count against brute force.  Built and run by tests/test_coalesce_gram.py under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "multi.hpp"

using sg::kGramCap;
using sg::kGramSlots;
typedef std::vector<uint8_t> Bytes;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 16) % below);
}

// the table as the workgroup's prologue builds it: default, then the least shift per slot, then the pattern bits
static std::vector<uint32_t> build(const std::vector<Bytes>& pats, uint32_t m)
{
    std::vector<uint32_t> S(kGramSlots, sg::gram_default(m));
    for (const Bytes& P : pats)
        for (uint32_t i = sg::gram_first(m); i + 3 <= m; ++i) {
            uint32_t& ent = S[sg::gram_slot(P[i], P[i + 1])];
            if (sg::gram_shift(m, i) < ent) ent = sg::gram_shift(m, i);
        }
    for (size_t g = 0; g < pats.size(); ++g) S[sg::gram_slot(pats[g][m - 2], pats[g][m - 1])] |= sg::gram_entry_pattern_bit((uint32_t)g);
    return S;
}

// counts of the walk; -1 in bad if an entry would not move the window end
static std::vector<uint64_t> walk(const Bytes& T, const std::vector<Bytes>& pats, uint32_t m, const std::vector<uint32_t>& S, int* bad)
{
    const uint32_t H = m - 1 < 16 ? m - 1 : 16;  // the bytes a lane compares in LDS before the rest in memory
    std::vector<uint64_t> counts(pats.size(), 0);
    const uint64_t e_begin = m - 1, e_end = T.size();
    for (uint64_t seg = 0; seg < e_end; seg += 64) {  // one lane's segment of window ends
        const uint64_t lo = seg > e_begin ? seg : e_begin, hi = seg + 64 < e_end ? seg + 64 : e_end;
        for (uint64_t e = lo; e < hi;) {
            const uint32_t ent = S[sg::gram_slot(T[e - 1], T[e])];
            for (uint32_t cand = sg::gram_entry_patterns(ent); cand; cand &= cand - 1) {
                const uint32_t g = (uint32_t)__builtin_ctz(cand);
                if (g >= pats.size()) { *bad = 1; continue; }
                const Bytes& P = pats[g];
                uint32_t k = 0;
                while (k <= H && P[m - 1 - k] == T[e - k]) ++k;
                if (k == H + 1 && std::memcmp(&T[e - (m - 1)], &P[0], m - 1 - H) == 0) ++counts[g];
            }
            if (sg::gram_entry_shift(ent) < 1 || sg::gram_entry_shift(ent) > sg::gram_default(m)) { *bad = 1; return counts; }
            e += sg::gram_entry_shift(ent);
        }
    }
    return counts;
}

static uint64_t brute(const Bytes& T, const Bytes& P)
{
    uint64_t c = 0;
    for (size_t s = 0; s + P.size() <= T.size(); ++s) c += std::memcmp(&T[s], &P[0], P.size()) == 0;
    return c;
}

static int g_cases = 0, g_failures = 0;

static void check(const char* what, uint32_t sigma, uint32_t m, const Bytes& T, const std::vector<Bytes>& pats, uint64_t at_least)
{
    int bad = 0;
    const std::vector<uint64_t> got = walk(T, pats, m, build(pats, m), &bad);
    ++g_cases;
    bool ok = !bad;
    for (size_t g = 0; g < pats.size(); ++g) {
        const uint64_t want = brute(T, pats[g]);
        ok = ok && got[g] == want && (g != 0 || want >= at_least);
    }
    if (!ok) {
        ++g_failures;
        std::printf("FAIL %s sigma %u m %u np %zu bad %d\n", what, sigma, m, pats.size(), bad);
    }
}

int main()
{
    const uint32_t N = 20000, sigmas[3] = {256, 128, 8}, ms[6] = {8, 9, 17, 18, 66, kGramCap + 36};
    static_assert(kGramCap + 36 > kGramCap + 2, "one length whose shifts are capped by more than a byte");
    for (uint32_t sigma : sigmas) {
        Bytes base(N);
        for (uint8_t& b : base) b = (uint8_t)rnd(sigma);
        for (uint32_t m : ms)
            for (uint32_t np = 1; np <= 8; ++np) {
                std::vector<Bytes> pats;
                for (uint32_t g = 0; g < np; ++g) {
                    const uint32_t k = rnd(N - m);
                    pats.push_back(Bytes(base.begin() + k, base.begin() + k + m));
                }
                check("cut", sigma, m, base, pats, 1);
                // pattern 0 with its end at every residue mod 64
                {
                    Bytes T = base;
                    const uint32_t blocks = (m + 63) / 64;  // copy r ends at 64 * (blocks + r * (blocks + 1)) + r: apart by m at least
                    for (uint32_t r = 0; r < 64; ++r) std::memcpy(&T[64 * (blocks + r * (blocks + 1)) + r - (m - 1)], &pats[0][0], m);
                    check("residues", sigma, m, T, pats, 64);
                }
                if (np >= 2) {
                    // every pattern ends in pattern 0's last gram; each is planted once
                    std::vector<Bytes> same = pats;
                    Bytes T = base;
                    for (uint32_t g = 0; g < np; ++g) {
                        same[g][m - 2] = pats[0][m - 2];
                        same[g][m - 1] = pats[0][m - 1];
                        std::memcpy(&T[100 + g * (m + 77)], &same[g][0], m);
                    }
                    check("same last gram", sigma, m, T, same, 1);
                    // two identical patterns: each gets its own count
                    std::vector<Bytes> twin = pats;
                    twin[np - 1] = twin[0];
                    check("identical", sigma, m, base, twin, 1);
                }
            }
    }
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures != 0;
}
