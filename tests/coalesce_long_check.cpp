// coalesce_long_check.cpp — a LONG pass of hor_multi_scan (smart_amd/csrc/multi.hpp: long_width) on the host, beside the
// by-value pass of the same length.  A long pass carries pointers only: every pattern lies at the front of a slot of
// kPatternSlot bytes, as in a plan's blob — here with 0xA5 behind the pattern, where a blob has zeros, so that a byte
// behind tail_stored(m) that mattered would show — and the rows are gathered from there in pieces of 16 bytes at
// blob + gram_first(m) + offset, as the kernel's prologue gathers them, into ONE heap buffer laid out as the kernel's
// LDS behind the heads: np rows | u32 next[np] | u32 sums[np], of exactly long_head() bytes less the table and the
// heads (the sanitizer guards both ends).  The byte table, the heads and the chains are built with the header's
// functions, a text is walked a lane's 64 window ends at a time, and every count must equal brute force.
// Per text (rand128, rand256; 512 KiB) and length (8, 16, 17, 32, 33, 64, 65, 100), at pass_width(m) and at
// long_width(m) patterns cut from the text, it prints the wave-steps per 4096 bytes (the longest lane of 64, averaged)
// and the share of all lane-steps that hit a slot: what a long pass's walk costs beside a by-value pass's, before any
// GPU is asked.  The long group also holds, planted: the same pattern at places 1 and W + 1, two patterns of one last
// gram (0 and W), a pattern at the last place LW - 1, and a pattern at place W + 2 planted as a periodic run
// (an occurrence every m bytes, 40 times).  Built and run by tests/test_coalesce_long.py under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "multi.hpp"

using sg::kGramBuckets;
using sg::kGramSlots;
typedef std::vector<uint8_t> Bytes;

constexpr uint32_t kPatternSlot = 4224;  // kernels.hpp kPatternBytes

// the widths the formula gives, worked out here once more: the area, a thread per pattern, the LDS at four per CU
constexpr uint32_t by_formula(uint32_t m)
{
    uint32_t np = 0;
    while (16 * (np + 1) <= 4032 && np + 1 <= 256 - 4 && 16384 + 4 * 512 + 8 * (np + 1) + (((np + 1) * sg::tail_stride(m) + 63) & ~63u) + 16448 <= 40960) ++np;
    return np;
}
static_assert(sg::long_width(8) == by_formula(8) && sg::long_width(16) == by_formula(16) && sg::long_width(17) == by_formula(17) &&
              sg::long_width(32) == by_formula(32) && sg::long_width(33) == by_formula(33) && sg::long_width(48) == by_formula(48) &&
              sg::long_width(49) == by_formula(49) && sg::long_width(64) == by_formula(64) && sg::long_width(65) == by_formula(65) &&
              sg::long_width(100) == by_formula(100) && sg::long_width(4200) == by_formula(4200), "long_width is the formula's");
static_assert(sg::long_width(16) == 252 && sg::long_width(32) == 152 && sg::long_width(48) == 108 && sg::long_width(64) == 84 && sg::long_width(65) == 68, "the long widths");
static_assert(sg::long_width(16) * 16 <= sg::kMultiArea && sg::kLongMax == 252, "two pointers per pattern fit the area");

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 16) % below);
}

static uint32_t halo(uint32_t m) { return m - 1 < 16 ? m - 1 : 16; }

struct Pass {
    uint32_t m, np, stride;
    std::unique_ptr<uint8_t[]> lds;  // rows | next | sums, rounded to 64 as long_head rounds
    std::vector<uint8_t> gram;
    std::vector<uint32_t> heads;
    const uint8_t* row(uint32_t g) const { return lds.get() + g * stride; }
    uint32_t* next() const { return reinterpret_cast<uint32_t*>(lds.get() + np * stride); }
};

// blobs[g]: a pattern slot.  long_layout: the rows gathered in 16-byte pieces from the slots into the long pass's LDS;
// otherwise packed from tail_fill rows as api.cpp packs a by-value pass.  Then the table and the chains.
static Pass build(const std::vector<Bytes>& blobs, uint32_t m, bool long_layout)
{
    Pass p;
    p.m = m;
    p.np = (uint32_t)blobs.size();
    p.stride = sg::tail_stride(m);
    const uint32_t bytes = sg::long_head(p.np, p.stride) - kGramSlots - 4 * kGramBuckets;
    p.lds.reset(new uint8_t[bytes]);
    std::memset(p.lds.get(), 0xEE, bytes);
    if (long_layout) {
        const uint32_t pieces = p.stride / 16, all = p.np * pieces;
        for (uint32_t x = 0; x < all; ++x) {  // thread x, and x + THREADS
            const uint32_t g = x / pieces;
            std::memcpy(p.lds.get() + x * 16, &blobs[g][0] + sg::gram_first(m) + (x - g * pieces) * 16, 16);
        }
    } else {
        for (uint32_t g = 0; g < p.np; ++g) {
            uint8_t full[sg::kTailRow];
            sg::tail_fill(full, &blobs[g][0], m);
            std::memcpy(p.lds.get() + g * p.stride, full, p.stride);
        }
    }
    p.gram.assign(kGramSlots, (uint8_t)sg::gram_default(m));
    for (uint32_t g = 0; g < p.np; ++g)
        for (uint32_t i = sg::gram_first(m); i + 3 <= m; ++i) {
            const uint32_t two = sg::tail_gram_at(p.row(g), m, i);
            uint8_t& ent = p.gram[sg::gram_slot(two & 0xFFu, two >> 8)];
            if (sg::gram_shift(m, i) < ent) ent = (uint8_t)sg::gram_shift(m, i);
        }
    p.heads.assign(kGramBuckets, 0);
    for (uint32_t g = 0; g < p.np; ++g) {
        const uint32_t two = sg::tail_gram_at(p.row(g), m, m - 2);
        p.gram[sg::gram_slot(two & 0xFFu, two >> 8)] |= sg::kGramHit;
        uint32_t& head = p.heads[sg::gram_bucket(two & 0xFFu, two >> 8)];
        p.next()[g] = head;
        p.next()[p.np + g] = 0;  // sums[g]
        head = g + 1;
    }
    return p;
}

struct Walk { uint64_t wave_steps = 0, lane_steps = 0, hits = 0; int bad = 0; };

static Walk walk(const Bytes& T, const std::vector<Bytes>& blobs, const Pass& p, std::vector<uint64_t>& counts)
{
    const uint32_t m = p.m, H = halo(m);
    Walk w;
    uint32_t* sums = p.next() + p.np;
    const uint64_t e_begin = m - 1, e_end = T.size();
    uint64_t wave_most = 0;
    for (uint64_t seg = 0; seg < e_end; seg += 64) {
        const uint64_t lo = seg > e_begin ? seg : e_begin, hi = seg + 64 < e_end ? seg + 64 : e_end;
        uint64_t mine = 0;
        for (uint64_t e = lo; e < hi; ++mine) {
            const uint32_t prev = T[e - 1], last = T[e];
            const uint32_t ent = p.gram[sg::gram_slot(prev, last)];
            if (sg::gram_byte_hit(ent)) {
                ++w.hits;
                uint32_t links = 0;
                for (uint32_t c = p.heads[sg::gram_bucket(prev, last)]; c != 0; c = p.next()[c - 1]) {
                    if (c > p.np || ++links > p.np) { w.bad = 1; return w; }
                    const uint32_t g = c - 1;
                    uint32_t k = 0;
                    while (k <= H && sg::tail_at(p.row(g), m, m - 1 - k) == T[e - k]) ++k;
                    if (k == H + 1 && std::memcmp(&T[e - (m - 1)], &blobs[g][0], m - 1 - H) == 0) ++sums[g];
                }
            }
            const uint32_t shift = sg::gram_byte_shift(ent);
            if (shift < 1 || shift > sg::gram_default(m)) { w.bad = 1; return w; }
            e += shift;
        }
        w.lane_steps += mine;
        if (mine > wave_most) wave_most = mine;
        if ((seg / 64) % 64 == 63 || seg + 64 >= e_end) {
            w.wave_steps += wave_most;
            wave_most = 0;
        }
    }
    counts.assign(sums, sums + p.np);
    return w;
}

static uint64_t brute(const Bytes& T, const uint8_t* P, uint32_t m)
{
    uint64_t c = 0;
    const uint8_t* at = &T[0];
    const uint8_t* const end = &T[0] + T.size() - m + 1;
    while (at < end && (at = (const uint8_t*)std::memchr(at, P[0], (size_t)(end - at))) != nullptr) {
        c += std::memcmp(at, P, m) == 0;
        ++at;
    }
    return c;
}

static int g_cases = 0, g_failures = 0;

static Walk check(const char* what, const char* text, uint32_t m, const Bytes& T, const std::vector<Bytes>& blobs, bool long_layout, const std::vector<uint64_t>& at_least)
{
    ++g_cases;
    const Pass p = build(blobs, m, long_layout);
    std::vector<uint64_t> got;
    const Walk w = walk(T, blobs, p, got);
    size_t wrong = 0;
    if (!w.bad)
        for (size_t g = 0; g < blobs.size(); ++g) {
            const uint64_t n = brute(T, &blobs[g][0], m);
            if (got[g] != n || n < at_least[g]) ++wrong;
        }
    if (w.bad || wrong) {
        ++g_failures;
        std::printf("FAIL %s %s m %u np %zu: %zu counts wrong, bad %d\n", what, text, m, blobs.size(), wrong, w.bad);
    }
    return w;
}

static Bytes slot_of(const uint8_t* P, uint32_t m)
{
    Bytes b(kPatternSlot, (uint8_t)0xA5);
    std::memcpy(&b[0], P, m);
    return b;
}

int main()
{
    const uint32_t N = 512u << 10, ms[8] = {8, 16, 17, 32, 33, 64, 65, 100};
    const char* names[2] = {"rand128", "rand256"};
    for (uint32_t text = 0; text < 2; ++text) {
        const uint32_t sigma = text == 0 ? 128 : 256;
        Bytes base(N);
        for (uint32_t j = 0; j < N; ++j) base[j] = (uint8_t)rnd(sigma);
        for (uint32_t m : ms) {
            const uint32_t W = sg::pass_width(m), LW = sg::long_width(m);
            if (LW <= W + 2) return 2;
            std::vector<Bytes> cut;
            for (uint32_t g = 0; g < LW; ++g) cut.push_back(slot_of(&base[rnd(N - m)], m));
            // the by-value pass of W and the long pass of LW over the same text: the model's figures
            const Walk a = check("by value", names[text], m, base, std::vector<Bytes>(cut.begin(), cut.begin() + W), false, std::vector<uint64_t>(W, 1));
            const Walk b = check("long", names[text], m, base, cut, true, std::vector<uint64_t>(LW, 1));
            const double waves = (double)((N + 4095) / 4096);
            std::printf("%-7s m %3u: np %3u %.2f wave-steps per 4096 bytes, %.3f %% of steps hit | np %3u %.2f, %.3f %%\n", names[text], m, W,
                        (double)a.wave_steps / waves, 100.0 * (double)a.hits / (double)a.lane_steps, LW, (double)b.wave_steps / waves,
                        100.0 * (double)b.hits / (double)b.lane_steps);
            // a long pass of W + 1 (the narrowest) in the long layout counts as well
            check("long, narrowest", names[text], m, base, std::vector<Bytes>(cut.begin(), cut.begin() + W + 1), true, std::vector<uint64_t>(W + 1, 1));
            // the special long group: fresh random patterns, planted
            std::vector<Bytes> sp = cut;
            const uint32_t fresh[6] = {0, 1, W, W + 1, W + 2, LW - 1};
            for (uint32_t g : fresh) {
                for (uint32_t j = 0; j < m; ++j) sp[g][j] = (uint8_t)rnd(sigma);
            }
            sp[W][m - 2] = sp[0][m - 2];  // one last gram, places 0 and W
            sp[W][m - 1] = sp[0][m - 1];
            sp[W + 1] = sp[1];            // one pattern, places 1 and W + 1
            Bytes T = base;
            std::vector<uint64_t> at_least(LW, 0);
            uint32_t at = 4096 + 77;
            for (uint32_t g : fresh) {
                std::memcpy(&T[at], &sp[g][0], m);
                at_least[g] = 1;
                at += 3 * 4096 + 131;
            }
            at_least[1] = at_least[W + 1] = 2;
            for (uint32_t r = 0; r < 40; ++r) std::memcpy(&T[200000 + 13 + r * m], &sp[W + 2][0], m);  // a periodic run
            at_least[W + 2] = 41;
            std::memcpy(&T[N - m], &sp[LW - 1][0], m);  // the last place at the last start position
            at_least[LW - 1] = 2;
            check("long, special", names[text], m, T, sp, true, at_least);
        }
    }
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures != 0;
}
