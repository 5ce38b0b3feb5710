// coalesce_tail_check.cpp — the rows that carry a pattern's end by value into hor_multi_scan (smart_amd/csrc/multi.hpp:
// kTailRow, tail_fill, tail_at) on the host: every row is filled by the rule into a heap buffer of exactly the row size,
// the skip table and the tails are built from the rows alone, as the kernel's prologue builds them, and must equal,
// entry by entry, those built from the whole patterns; a text walked with them, 64 window ends at a time, counts like
// brute force.  Built and run by tests/test_coalesce_tail.py under AddressSanitizer and UBSan: a read before a row's
// first stored byte or behind the row ends the program.  `coalesce_tail_check before-row` makes that read on purpose.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "multi.hpp"

using sg::kGramCap;
using sg::kGramSlots;
using sg::kTailRow;
typedef std::vector<uint8_t> Bytes;
typedef std::unique_ptr<uint8_t[]> Row;

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint32_t rnd(uint32_t below)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 16) % below);
}

static uint32_t halo(uint32_t m) { return m - 1 < 16 ? m - 1 : 16; }  // the bytes a lane compares in LDS: H = min(m - 1, 16)

static Row row_of(const Bytes& P)
{
    Row row(new uint8_t[kTailRow]);  // exactly the row: the sanitizer guards both ends
    sg::tail_fill(row.get(), &P[0], (uint32_t)P.size());
    return row;
}

// the table from the whole patterns (as tests/coalesce_gram_check.cpp builds it, and the tags of the last grams) ...
static std::vector<uint32_t> table_of_patterns(const std::vector<Bytes>& pats, uint32_t m)
{
    std::vector<uint32_t> S(kGramSlots, sg::gram_default(m));
    for (const Bytes& P : pats)
        for (uint32_t i = sg::gram_first(m); i + 3 <= m; ++i) {
            uint32_t& ent = S[sg::gram_slot(P[i], P[i + 1])];
            if (sg::gram_shift(m, i) < ent) ent = sg::gram_shift(m, i);
        }
    for (size_t g = 0; g < pats.size(); ++g) S[sg::gram_slot(pats[g][m - 2], pats[g][m - 1])] |= sg::gram_entry_pattern_bit((uint32_t)g) | sg::gram_entry_tag(pats[g][m - 2]);
    return S;
}

// ... and from the rows, as the kernel's prologue does: position gram_first(m) + x % kGramCap of pattern x / kGramCap
static std::vector<uint32_t> table_of_rows(const std::vector<Row>& rows, uint32_t m)
{
    std::vector<uint32_t> S(kGramSlots, sg::gram_default(m));
    for (uint32_t x = 0; x < rows.size() * kGramCap; ++x) {
        const uint32_t i = sg::gram_first(m) + x % kGramCap;
        if (i + 3 > m) continue;
        const uint8_t* row = rows[x / kGramCap].get();
        uint32_t& ent = S[sg::gram_slot(sg::tail_at(row, m, i), sg::tail_at(row, m, i + 1))];
        if (sg::gram_shift(m, i) < ent) ent = sg::gram_shift(m, i);
    }
    for (size_t g = 0; g < rows.size(); ++g)
        S[sg::gram_slot(sg::tail_at(rows[g].get(), m, m - 2), sg::tail_at(rows[g].get(), m, m - 1))] |= sg::gram_entry_pattern_bit((uint32_t)g) | sg::gram_entry_tag(sg::tail_at(rows[g].get(), m, m - 2));
    return S;
}

// a pattern's tail as a lane compares it: tail[j] == P[m-1-H+j], j <= H
static Bytes tail_of_row(const uint8_t* row, uint32_t m)
{
    const uint32_t H = halo(m);
    Bytes t(H + 1);
    for (uint32_t j = 0; j <= H; ++j) t[j] = (uint8_t)sg::tail_at(row, m, m - 1 - H + j);
    return t;
}

// counts of the walk over table S: the last H + 1 bytes against the tails, the rest against the pattern in memory
static std::vector<uint64_t> walk(const Bytes& T, const std::vector<Bytes>& pats, const std::vector<Bytes>& tails, uint32_t m, const std::vector<uint32_t>& S, int* bad)
{
    const uint32_t H = halo(m);
    std::vector<uint64_t> counts(pats.size(), 0);
    const uint64_t e_begin = m - 1, e_end = T.size();
    for (uint64_t seg = 0; seg < e_end; seg += 64) {  // one lane's segment of window ends
        const uint64_t lo = seg > e_begin ? seg : e_begin, hi = seg + 64 < e_end ? seg + 64 : e_end;
        for (uint64_t e = lo; e < hi;) {
            const uint32_t ent = S[sg::gram_slot(T[e - 1], T[e])];
            for (uint32_t cand = sg::gram_entry_hit(ent, T[e - 1]); cand; cand &= cand - 1) {  // no compare where the slot is hit and the gram is not
                const uint32_t g = (uint32_t)__builtin_ctz(cand);
                if (g >= pats.size()) { *bad = 1; continue; }
                uint32_t k = 0;
                while (k <= H && tails[g][H - k] == T[e - k]) ++k;
                if (k == H + 1 && std::memcmp(&T[e - (m - 1)], &pats[g][0], m - 1 - H) == 0) ++counts[g];
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

static void check(const char* what, uint32_t m, const Bytes& T, const std::vector<Bytes>& pats, uint64_t at_least)
{
    ++g_cases;
    const uint32_t H = halo(m);
    std::vector<Row> rows;
    for (const Bytes& P : pats) rows.push_back(row_of(P));
    bool ok = true;
    // the rows: the stored bytes, zeros behind them
    for (size_t g = 0; g < pats.size(); ++g)
        for (uint32_t j = 0; j < kTailRow; ++j) ok = ok && rows[g][j] == (j < sg::tail_stored(m) ? pats[g][sg::gram_first(m) + j] : 0);
    // tails and table from the rows against those from the patterns
    std::vector<Bytes> tails;
    for (size_t g = 0; g < pats.size(); ++g) {
        tails.push_back(tail_of_row(rows[g].get(), m));
        ok = ok && std::memcmp(&tails[g][0], &pats[g][m - 1 - H], H + 1) == 0;
    }
    const std::vector<uint32_t> S = table_of_rows(rows, m), want = table_of_patterns(pats, m);
    uint32_t differ = 0;
    for (uint32_t s = 0; s < kGramSlots; ++s) differ += S[s] != want[s];
    ok = ok && differ == 0;
    int bad = 0;
    const std::vector<uint64_t> got = walk(T, pats, tails, m, S, &bad);
    ok = ok && !bad;
    for (size_t g = 0; g < pats.size(); ++g) {
        const uint64_t n = brute(T, pats[g]);
        ok = ok && got[g] == n && (g != 0 || n >= at_least);
    }
    if (!ok) {
        ++g_failures;
        std::printf("FAIL %s m %u np %zu: %u table entries differ, bad %d\n", what, m, pats.size(), differ, bad);
    }
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "before-row") == 0) {  // the byte in front of a row's first: the sanitizer must end the program
        const uint32_t m = 100;
        const Row row = row_of(Bytes(m, 7));
        const uint32_t b = sg::tail_at(row.get(), m, sg::gram_first(m) - 1);
        std::printf("read %u in front of the row\n", b);
        return 0;
    }
    static_assert(sg::kTailRow % 16 == 0 && sg::kTailRow >= kGramCap + 1, "a row is padded to 16 bytes and holds kGramCap + 1 of them");
    const uint32_t N = 20000, ms[10] = {3, 8, 17, 18, 64, 65, 66, 67, 100, 4096};
    Bytes base(N);
    for (uint8_t& b : base) b = (uint8_t)rnd(256);
    for (uint32_t m : ms)
        for (uint32_t np = 1; np <= 8; ++np) {
            std::vector<Bytes> pats;
            for (uint32_t g = 0; g < np; ++g) {
                const uint32_t k = rnd(N - m);
                pats.push_back(Bytes(base.begin() + k, base.begin() + k + m));
            }
            check("cut", m, base, pats, 1);
            if (np >= 2) {
                // every pattern ends in pattern 0's last gram and is planted once, as far as the text has room (pattern 0
                // always is); the last one is pattern 0 again
                std::vector<Bytes> same = pats;
                same[np - 1] = same[0];
                Bytes T = base;
                for (uint32_t g = 0; g < np; ++g) {
                    same[g][m - 2] = pats[0][m - 2];
                    same[g][m - 1] = pats[0][m - 1];
                    if (100 + g * (m + 77) + m <= N) std::memcpy(&T[100 + g * (m + 77)], &same[g][0], m);
                }
                check("same last gram", m, T, same, 100 + (np - 1) * (m + 77) + m <= N ? 2 : 1);
            }
        }
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures != 0;
}
