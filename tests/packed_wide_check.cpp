// packed_wide_check.cpp — what the calls on a three-plane packed text decide on the host (smart_amd/csrc/planes3_host.hpp),
// without a device: every bit of the eight membership planes that encode_sets8 and encode_pattern8 write against the
// definition in planes3.hpp, with their counts and flags.  Built and run by tests/test_packed_wide_host.py under
// AddressSanitizer and UBSan; every buffer is a heap block of exactly the documented size.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "planes3_host.hpp"

using sg::kPatWords;
using sg::kSet8Words;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 16) % below);
}

static int g_cases = 0, g_failures = 0;
static void check(bool ok, const char* what, int a, int b, int c, int d)
{
    ++g_cases;
    if (ok) return;
    ++g_failures;
    printf("FAILED %s (%d, %d, %d, %d)\n", what, a, b, c, d);
}

static bool bit(const uint32_t* Y, uint32_t c, uint32_t j) { return Y[c * kPatWords + (j >> 5)] >> (j & 31) & 1u; }

static const uint32_t kLengths[7] = {1, 31, 32, 33, 64, 65, SMARTGPU_XSIZE};
static const int kAlphabets[3] = {5, 6, 8};

// By definition: position j < m has bit c when its set holds c; the full set and — when filled — the empty set have all
// eight; nothing is set from m to the planes' end.
static bool planes_match(const uint32_t* Y, const std::vector<uint8_t>& sets, uint32_t all, bool fill)
{
    const uint32_t m = (uint32_t)sets.size();
    for (uint32_t j = 0; j < 32 * kPatWords; ++j) {
        uint32_t want = 0;
        if (j < m) want = sets[j] == all || (sets[j] == 0 && fill) ? 0xFFu : sets[j];
        for (uint32_t c = 0; c < 8; ++c)
            if (bit(Y, c, j) != ((want >> c & 1u) != 0)) return false;
    }
    return true;
}

// encode_sets8: nvalues x m x {empty positions kept, filled} x {a mix with empty, full and singleton positions, all full,
// neither empty nor all full}; then a set with a bit at or above nvalues, twice: the first is reported (nvalues < 8 only:
// with eight values every bit is a code)
static void set_cases()
{
    for (int nvalues : kAlphabets)
        for (uint32_t m : kLengths)
            for (int fill = 0; fill < 2; ++fill) {
                const uint32_t all = (1u << nvalues) - 1u;
                for (int kind = 0; kind < 3; ++kind) {
                    std::vector<uint8_t> sets(m);
                    for (uint32_t j = 0; j < m; ++j) {
                        const uint32_t r = rnd(4);
                        sets[j] = (uint8_t)(kind == 1 ? all : kind == 2 ? 1 + rnd(all - 1) : r == 0 ? 0 : r == 1 ? all : r == 2 ? 1u << rnd(nvalues) : rnd(all + 1));
                    }
                    if (kind == 0) sets[m - 1] = 0;  // the last position among the empty ones
                    uint32_t want_empty = 0;
                    bool want_full = true;
                    for (uint32_t j = 0; j < m; ++j) {
                        want_empty += sets[j] == 0;
                        want_full = want_full && sets[j] == all;
                    }
                    std::vector<uint32_t> Y(kSet8Words, 0xA5A5A5A5u);
                    uint32_t empty = 77;
                    bool full = !want_full;
                    const int bad = sg::encode_sets8(nvalues, sets.data(), m, fill != 0, Y.data(), &empty, &full);
                    check(bad == -1 && empty == want_empty && full == want_full && planes_match(Y.data(), sets, all, fill != 0), "encode_sets8", nvalues,
                          (int)m, fill, kind);
                }
                if (nvalues == 8) continue;
                std::vector<uint8_t> sets(m, 1);
                const uint32_t first = rnd(m);
                sets[first] = (uint8_t)(1u << nvalues);
                sets[m - 1] = (uint8_t)(sets[m - 1] | 0x80u);
                std::vector<uint32_t> Y(kSet8Words);
                uint32_t empty = 0;
                bool full = false;
                check(sg::encode_sets8(nvalues, sets.data(), m, fill != 0, Y.data(), &empty, &full) == (int)first, "encode_sets8 bad set", nvalues, (int)m,
                      fill, (int)first);
            }
}

// pattern_sets8 and encode_pattern8: nvalues x m x {0, 1, several foreign bytes} x {foreign positions kept empty, filled}
static void pattern_cases()
{
    for (int nvalues : kAlphabets)
        for (uint32_t m : kLengths)
            for (int kind = 0; kind < 3; ++kind)
                for (int fill = 0; fill < 2; ++fill) {
                    uint8_t values[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ascending and distinct, none of them 255 (the foreign byte below)
                    for (int k = 0; k < nvalues; ++k) values[k] = (uint8_t)((k ? values[k - 1] + 1 : 0) + rnd(25));
                    std::vector<uint8_t> P(m), want(m);
                    for (uint32_t j = 0; j < m; ++j) {
                        const uint32_t c = rnd(nvalues);
                        P[j] = values[c];
                        want[j] = (uint8_t)(1u << c);
                    }
                    uint32_t want_foreign = 0;
                    for (int f = 0; f < (kind == 2 ? 5 : kind); ++f) {
                        const uint32_t j = f == 0 ? m - 1 : rnd(m);  // the last position among them
                        if (want[j]) ++want_foreign;
                        want[j] = 0;
                        P[j] = 255;
                    }
                    std::vector<uint8_t> sets(m, 0xEE);
                    bool ok = sg::pattern_sets8(values, nvalues, P.data(), m, sets.data()) == want_foreign && sets == want;
                    std::vector<uint32_t> Y(kSet8Words, 0x5A5A5A5Au);
                    ok = ok && sg::encode_pattern8(values, nvalues, P.data(), m, fill != 0, Y.data()) == want_foreign;
                    ok = ok && planes_match(Y.data(), want, (1u << nvalues) - 1u, fill != 0);
                    check(ok, "encode_pattern8", nvalues, (int)m, kind, fill);
                }
}

int main()
{
    set_cases();
    pattern_cases();
    printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures != 0;
}
