// coalesce_pass_check.cpp — a shared pass of up to kPassMax = 96 patterns (smart_amd/csrc/multi.hpp) on the host: the rows
// of a pass are packed at the stride of their length into a heap buffer of exactly np x stride bytes, the BYTE skip table
// (shift in bits 0-6, hit bit 7), the bucket heads and the chains are built from those rows with the header's functions,
// in the order the kernel's prologue builds them, and a text is walked as hor_multi_scan walks it — a lane's 64 window
// ends at a time; a window whose entry has the hit bit follows the chain of its gram's bucket and is compared, whole,
// with every pattern on it — and every pattern's count must equal brute force.  Every shift taken lies in
// [1, gram_default(m)].  Texts of 20 000 bytes: rand128, rand256 (bytes >= 128: slots alias) and a periodic text of
// two symbols; m = 3, 8, 17, 18, 33, 64, 65, 66, 100; groups of 1, 2, 31, 32, 33, the widest pass of the length and one
// below it; from eight patterns on also a group that holds two patterns with one last gram (0 and 2), two patterns in
// one bucket with different last grams (3 and 4), the same pattern twice (1 and 5) and a pattern whose last gram is
// another's inner gram (6 and 7), all planted.  It prints, per text and length, the wave-steps of the widest pass: the
// longest lane of 64, averaged.  Built and run by tests/test_coalesce_pass.py under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "multi.hpp"

using sg::kGramBuckets;
using sg::kGramSlots;
using sg::kPassMax;
typedef std::vector<uint8_t> Bytes;

static_assert(sg::pass_width(16) == 96 && sg::pass_width(17) == 84 && sg::pass_width(32) == 84 && sg::pass_width(64) == 50 && sg::pass_width(65) == 42,
              "the widest pass: the area over two pointers and a row of round16(min(m, 65)) bytes");
static_assert(sizeof(sg::MultiArgs) == 4080 && sizeof(sg::MultiArgs) + 8 + 4 <= 4096 && sg::kMultiArea == 4032, "the arguments of a pass");
static_assert(sg::pass_width(65) * (16 + sg::tail_stride(65)) <= sg::kMultiArea && sg::pass_width(32) * (16 + sg::tail_stride(32)) <= sg::kMultiArea &&
              (uint32_t)kPassMax * (16 + sg::tail_stride(16)) <= sg::kMultiArea, "the widest pass fits the area");

static uint64_t g_rng = 0xA0761D6478BD642Full;
static uint32_t rnd(uint32_t below)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 16) % below);
}

static uint32_t halo(uint32_t m) { return m - 1 < 16 ? m - 1 : 16; }  // the bytes a lane compares in LDS: H = min(m - 1, 16)

struct Pass {
    uint32_t m, np, stride;
    std::unique_ptr<uint8_t[]> rows;  // exactly np x stride bytes: the sanitizer guards both ends
    std::vector<uint8_t> gram;        // kGramSlots byte entries
    std::vector<uint32_t> heads, next;
    const uint8_t* row(uint32_t g) const { return rows.get() + g * stride; }
};

// the rows as api.cpp packs them (the first `stride` bytes of what tail_fill leaves), then the table and the chains
// as the kernel's prologue builds them: the default, the least shift per slot, the hit bits and the links
static Pass build(const std::vector<Bytes>& pats, uint32_t m)
{
    Pass p;
    p.m = m;
    p.np = (uint32_t)pats.size();
    p.stride = sg::tail_stride(m);
    p.rows.reset(new uint8_t[p.np * p.stride]);
    for (uint32_t g = 0; g < p.np; ++g) {
        uint8_t full[sg::kTailRow];
        sg::tail_fill(full, &pats[g][0], m);
        std::memcpy(p.rows.get() + g * p.stride, full, p.stride);
    }
    p.gram.assign(kGramSlots, (uint8_t)sg::gram_default(m));
    for (uint32_t g = 0; g < p.np; ++g)
        for (uint32_t i = sg::gram_first(m); i + 3 <= m; ++i) {
            const uint32_t two = sg::tail_gram_at(p.row(g), m, i);
            uint8_t& ent = p.gram[sg::gram_slot(two & 0xFFu, two >> 8)];
            if (sg::gram_shift(m, i) < ent) ent = (uint8_t)sg::gram_shift(m, i);
        }
    p.heads.assign(kGramBuckets, 0);
    p.next.assign(p.np, 0);
    for (uint32_t g = 0; g < p.np; ++g) {
        const uint32_t two = sg::tail_gram_at(p.row(g), m, m - 2);
        p.gram[sg::gram_slot(two & 0xFFu, two >> 8)] |= sg::kGramHit;
        uint32_t& head = p.heads[sg::gram_bucket(two & 0xFFu, two >> 8)];
        p.next[g] = head;
        head = g + 1;
    }
    return p;
}

// counts of the walk; *bad: a shift out of range or a chain that does not end; *steps: wave-steps — per 64 lanes, the
// steps of the one that takes most — summed
static std::vector<uint64_t> walk(const Bytes& T, const std::vector<Bytes>& pats, const Pass& p, int* bad, uint64_t* steps)
{
    const uint32_t m = p.m, H = halo(m);
    std::vector<uint64_t> counts(p.np, 0);
    const uint64_t e_begin = m - 1, e_end = T.size();
    uint64_t wave_most = 0;
    for (uint64_t seg = 0; seg < e_end; seg += 64) {  // one lane's segment of window ends
        const uint64_t lo = seg > e_begin ? seg : e_begin, hi = seg + 64 < e_end ? seg + 64 : e_end;
        uint64_t mine = 0;
        for (uint64_t e = lo; e < hi; ++mine) {
            const uint32_t prev = T[e - 1], last = T[e];
            const uint32_t ent = p.gram[sg::gram_slot(prev, last)];
            if (sg::gram_byte_hit(ent)) {
                uint32_t links = 0;
                for (uint32_t c = p.heads[sg::gram_bucket(prev, last)]; c != 0; c = p.next[c - 1]) {
                    if (c > p.np || ++links > p.np) { *bad = 1; return counts; }
                    const uint32_t g = c - 1;
                    uint32_t k = 0;  // the last H + 1 bytes against the row, the rest against the pattern in memory
                    while (k <= H && sg::tail_at(p.row(g), m, m - 1 - k) == T[e - k]) ++k;
                    if (k == H + 1 && std::memcmp(&T[e - (m - 1)], &pats[g][0], m - 1 - H) == 0) ++counts[g];
                }
            }
            const uint32_t shift = sg::gram_byte_shift(ent);
            if (shift < 1 || shift > sg::gram_default(m)) { *bad = 1; return counts; }
            e += shift;
        }
        if (mine > wave_most) wave_most = mine;
        if ((seg / 64) % 64 == 63 || seg + 64 >= e_end) {
            *steps += wave_most;
            wave_most = 0;
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

// at_least[g]: occurrences pattern g has at the least (planted copies).  Returns wave-steps per wave.
static double check(const char* what, const char* text, uint32_t m, const Bytes& T, const std::vector<Bytes>& pats, const std::vector<uint64_t>& at_least)
{
    ++g_cases;
    const Pass p = build(pats, m);
    bool ok = true;
    for (uint32_t s = 0; s < kGramSlots; ++s) ok = ok && sg::gram_byte_shift(p.gram[s]) >= 1 && sg::gram_byte_shift(p.gram[s]) <= sg::gram_default(m);
    int bad = 0;
    uint64_t steps = 0;
    const std::vector<uint64_t> got = walk(T, pats, p, &bad, &steps);
    ok = ok && !bad;
    size_t wrong = 0;
    for (size_t g = 0; g < pats.size(); ++g) {
        const uint64_t n = brute(T, pats[g]);
        if (got[g] != n || n < at_least[g]) ++wrong;
    }
    if (!ok || wrong) {
        ++g_failures;
        std::printf("FAIL %s %s m %u np %zu: %zu counts wrong, bad %d\n", what, text, m, pats.size(), wrong, bad);
    }
    return (double)steps / (double)((T.size() + 4095) / 4096);
}

// a last gram other than (p0, l0) whose slot differs and whose bucket is the same; symbols below `sigma`
static bool bucket_mate(uint32_t sigma, uint32_t p0, uint32_t l0, uint32_t* prev, uint32_t* last)
{
    for (uint32_t a = 0; a < sigma; ++a)
        for (uint32_t b = 0; b < sigma; ++b)
            if (sg::gram_slot(a, b) != sg::gram_slot(p0, l0) && sg::gram_bucket(a, b) == sg::gram_bucket(p0, l0)) {
                *prev = a;
                *last = b;
                return true;
            }
    return false;
}

int main()
{
    // the slot function: exact on symbols below 128, and slot and prev determine last
    {
        std::vector<uint8_t> seen(kGramSlots, 0);
        for (uint32_t a = 0; a < 128; ++a)
            for (uint32_t b = 0; b < 128; ++b) {
                if (seen[sg::gram_slot(a, b)]++) return 2;
            }
        for (uint32_t a = 0; a < 256; ++a)
            for (uint32_t b = 0; b < 256; ++b) {
                if (sg::gram_slot(a, b) >= kGramSlots || sg::gram_bucket(a, b) >= kGramBuckets) return 2;
                if (((sg::gram_slot(a, b) - sg::gram_slot(a, 0)) & (kGramSlots - 1)) != b) return 2;
                if (a >= 128 && sg::gram_slot(a, b) == sg::gram_slot(a - 128, b)) return 2;
            }
    }
    const uint32_t N = 20000, ms[9] = {3, 8, 17, 18, 33, 64, 65, 66, 100};
    const char* names[3] = {"rand128", "rand256", "periodic2"};
    for (uint32_t text = 0; text < 3; ++text) {
        Bytes base(N);
        for (uint32_t j = 0; j < N; ++j) base[j] = text == 0 ? (uint8_t)rnd(128) : text == 1 ? (uint8_t)rnd(256) : (uint8_t)("ab"[(j % 7) % 2 ^ (j % 3 == 0)]);
        const uint32_t sigma = text == 1 ? 256 : 128;
        for (uint32_t m : ms) {
            const uint32_t W = sg::pass_width(m);
            const uint32_t groups[7] = {1, 2, 31, 32, 33, W, W - 1};
            for (uint32_t np : groups) {
                std::vector<Bytes> pats;
                for (uint32_t g = 0; g < np; ++g) {
                    const uint32_t k = rnd(N - m);
                    pats.push_back(Bytes(base.begin() + k, base.begin() + k + m));
                }
                const double steps = check("cut", names[text], m, base, pats, std::vector<uint64_t>(np, 1));
                if (np == W) std::printf("%-9s m %3u np %2u: %.2f wave-steps per 4096 bytes\n", names[text], m, np, steps);
                if (np < 8 || m < 8) continue;
                // the special group, of fresh random patterns so that nothing but what is planted ties them together
                std::vector<Bytes> sp = pats;
                for (uint32_t g = 0; g < 8; ++g)
                    for (uint8_t& b : sp[g]) b = (uint8_t)rnd(sigma);
                sp[2][m - 2] = sp[0][m - 2];  // one last gram, two patterns
                sp[2][m - 1] = sp[0][m - 1];
                uint32_t a = 0, b = 0;
                if (!bucket_mate(sigma, sp[3][m - 2], sp[3][m - 1], &a, &b)) return 3;
                sp[4][m - 2] = (uint8_t)a;    // one bucket, two last grams
                sp[4][m - 1] = (uint8_t)b;
                sp[5] = sp[1];                // the same pattern twice
                sp[7][m - 5] = sp[6][m - 2];  // the last gram of 6 is an inner gram of 7
                sp[7][m - 4] = sp[6][m - 1];
                Bytes T = base;
                std::vector<uint64_t> at_least(np, 0);
                for (uint32_t g = 0; g < 8; ++g) {
                    std::memcpy(&T[50 + g * 300], &sp[g][0], m);
                    at_least[g] = 1;
                }
                at_least[1] = at_least[5] = 2;
                check("special", names[text], m, T, sp, at_least);
            }
        }
    }
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures != 0;
}
