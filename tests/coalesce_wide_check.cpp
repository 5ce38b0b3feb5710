// coalesce_wide_check.cpp — a shared pass of up to kMultiMax = 32 patterns (smart_amd/csrc/multi.hpp) on the host: the
// skip table is built from rows filled by tail_fill, with a CLASS bit (gram_entry_class_bit) per pattern, and a text is
// walked as hor_multi_scan walks it — a lane's 64 window ends at a time, the tag test, then for every class bit of the
// entry the patterns c, c + 8, c + 16, c + 24 below np, each compared whole — and every pattern's count must equal
// brute force.  Every shift taken is checked to lie in [1, gram_default(m)].  Texts: 20 000 bytes of rand8, rand128 and
// rand256; m = 3, 8, 17, 18, 33, 66, 100; groups of 1 to 32 cut from the text, and from ten patterns on a group with
// two different patterns of one class that end in the same gram (0 and 8), the same whole pattern twice in one class
// (1 and 9) and the same last gram in two classes (0 and 2), all planted.  Built and run by tests/test_coalesce_wide.py
// under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "multi.hpp"

using sg::kGramSlots;
using sg::kMultiMax;
using sg::kTailRow;
typedef std::vector<uint8_t> Bytes;
typedef std::unique_ptr<uint8_t[]> Row;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 16) % below);
}

static uint32_t halo(uint32_t m) { return m - 1 < 16 ? m - 1 : 16; }  // the bytes a lane compares in LDS: H = min(m - 1, 16)

// the table as the kernel's prologue builds it: from the rows alone, shifts first, then class bits and tags
static std::vector<uint32_t> table_of_rows(const std::vector<Row>& rows, uint32_t m)
{
    std::vector<uint32_t> S(kGramSlots, sg::gram_default(m));
    for (const Row& row : rows)
        for (uint32_t i = sg::gram_first(m); i + 3 <= m; ++i) {
            const uint32_t two = sg::tail_gram_at(row.get(), m, i);
            uint32_t& ent = S[sg::gram_slot(two & 0xFFu, two >> 8)];
            if (sg::gram_shift(m, i) < ent) ent = sg::gram_shift(m, i);
        }
    for (size_t g = 0; g < rows.size(); ++g) {
        const uint32_t two = sg::tail_gram_at(rows[g].get(), m, m - 2);
        S[sg::gram_slot(two & 0xFFu, two >> 8)] |= sg::gram_entry_class_bit((uint32_t)g) | sg::gram_entry_tag(two & 0xFFu);
    }
    return S;
}

// counts of the walk over S; *compares: whole-pattern compares started; *bad: a shift out of range or a class bit above 7
static std::vector<uint64_t> walk(const Bytes& T, const std::vector<Bytes>& pats, const std::vector<Row>& rows, uint32_t m, const std::vector<uint32_t>& S,
                                  uint64_t* compares, int* bad)
{
    const uint32_t H = halo(m), np = (uint32_t)pats.size();
    std::vector<uint64_t> counts(np, 0);
    const uint64_t e_begin = m - 1, e_end = T.size();
    for (uint64_t seg = 0; seg < e_end; seg += 64) {  // one lane's segment of window ends
        const uint64_t lo = seg > e_begin ? seg : e_begin, hi = seg + 64 < e_end ? seg + 64 : e_end;
        for (uint64_t e = lo; e < hi;) {
            const uint32_t ent = S[sg::gram_slot(T[e - 1], T[e])];
            for (uint32_t cls = sg::gram_entry_hit(ent, T[e - 1]); cls; cls &= cls - 1) {
                const uint32_t c = (uint32_t)__builtin_ctz(cls);
                if (c >= sg::kGramClasses) { *bad = 1; continue; }
                for (uint32_t g = c; g < np; g += sg::kGramClasses) {
                    ++*compares;
                    uint32_t k = 0;  // the last H + 1 bytes against the row, the rest against the pattern in memory
                    while (k <= H && sg::tail_at(rows[g].get(), m, m - 1 - k) == T[e - k]) ++k;
                    if (k == H + 1 && std::memcmp(&T[e - (m - 1)], &pats[g][0], m - 1 - H) == 0) ++counts[g];
                }
            }
            const uint32_t shift = sg::gram_entry_shift(ent);
            if (shift < 1 || shift > sg::gram_default(m)) { *bad = 1; return counts; }
            e += shift;
        }
    }
    return counts;
}

static uint64_t brute(const Bytes& T, const Bytes& P)
{
    uint64_t c = 0;
    for (size_t s = 0; s + P.size() <= T.size(); ++s) c += T[s] == P[0] && std::memcmp(&T[s], &P[0], P.size()) == 0;
    return c;
}

static int g_cases = 0, g_failures = 0;

// at_least[g]: occurrences pattern g has at the least (planted copies)
static void check(const char* what, uint32_t sigma, uint32_t m, const Bytes& T, const std::vector<Bytes>& pats, const std::vector<uint64_t>& at_least)
{
    ++g_cases;
    std::vector<Row> rows;
    for (const Bytes& P : pats) {
        rows.emplace_back(new uint8_t[kTailRow]);  // exactly the row: the sanitizer guards both ends
        sg::tail_fill(rows.back().get(), &P[0], m);
    }
    const std::vector<uint32_t> S = table_of_rows(rows, m);
    bool ok = true;
    for (uint32_t s = 0; s < kGramSlots; ++s) ok = ok && sg::gram_entry_shift(S[s]) >= 1 && sg::gram_entry_shift(S[s]) <= sg::gram_default(m);
    int bad = 0;
    uint64_t compares = 0;
    const std::vector<uint64_t> got = walk(T, pats, rows, m, S, &compares, &bad);
    ok = ok && !bad;
    size_t wrong = 0;
    for (size_t g = 0; g < pats.size(); ++g) {
        const uint64_t n = brute(T, pats[g]);
        if (got[g] != n || n < at_least[g]) ++wrong;
    }
    if (!ok || wrong) {
        ++g_failures;
        std::printf("FAIL %s rand%u m %u np %zu: %zu counts wrong, bad %d, %llu compares\n", what, sigma, m, pats.size(), wrong, bad, (unsigned long long)compares);
    }
}

int main()
{
    static_assert(kMultiMax == 32 && sg::kGramClasses == 8, "four patterns to a class bit");
    for (uint32_t g = 0; g < (uint32_t)kMultiMax; ++g)  // pattern g sets bit g & 7: nothing changes below 8
        if (sg::gram_entry_class_bit(g) != sg::gram_entry_pattern_bit(g & 7u)) return 2;
    const uint32_t N = 20000, sigmas[3] = {8, 128, 256}, ms[7] = {3, 8, 17, 18, 33, 66, 100};
    for (uint32_t sigma : sigmas) {
        Bytes base(N);
        for (uint8_t& b : base) b = (uint8_t)rnd(sigma);
        for (uint32_t m : ms)
            for (uint32_t np = 1; np <= (uint32_t)kMultiMax; ++np) {
                std::vector<Bytes> pats;
                for (uint32_t g = 0; g < np; ++g) {
                    const uint32_t k = rnd(N - m);
                    pats.push_back(Bytes(base.begin() + k, base.begin() + k + m));
                }
                check("cut", sigma, m, base, pats, std::vector<uint64_t>(np, 1));
                if (np < 10) continue;
                std::vector<Bytes> mates = pats;
                for (uint32_t g : {2u, 8u}) {  // pattern 0's last gram in another class (2) and in its own (8)
                    mates[g][m - 2] = pats[0][m - 2];
                    mates[g][m - 1] = pats[0][m - 1];
                }
                mates[9] = mates[1];  // one pattern in two slots of a class: both get the whole count
                Bytes T = base;
                std::vector<uint64_t> at_least(np, 0);
                for (uint32_t g = 0; g < np; ++g) {
                    std::memcpy(&T[50 + g * 300], &mates[g][0], m);  // 50 + 31 * 300 + 100 <= N
                    at_least[g] = 1;
                }
                at_least[1] = at_least[9] = 2;
                check("class mates", sigma, m, T, mates, at_least);
            }
    }
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures != 0;
}
