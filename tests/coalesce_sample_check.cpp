// coalesce_sample_check.cpp — a pass of hor_sample_scan (smart_amd/csrc/sample.hpp, k_hors.hip) on the host.  The sample
// of a text is taken as text_sample_build takes it (dword k = T[28k .. 28k + 4), zeros from the pad), the bit filter,
// the heads and the entries are built from head rows with the header's own functions, the quads of a range are walked as
// the kernel walks them — filter bit, chain, gram compare, sample_window, the whole window in the text — and every count
// must equal brute force.  Per cell it prints the share of samples that pass the filter (profiles/coalesce/RESULTS.md
// quotes it).  Built and run by tests/test_coalesce_sample.py, plainly and under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sample.hpp"

typedef std::vector<uint8_t> Bytes;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 16) % below);
}

constexpr uint64_t kStep = 2800;  // a multiple of 28 between planted copies: copy r lies at residue (2048 + r) mod 28
constexpr uint32_t kPad = 64;  // zeros behind the text: the last sampled grams reach past n

struct Pass {
    uint32_t m = 0;
    std::vector<Bytes> pats;
    std::vector<uint32_t> filter, heads;
    std::vector<sg::SampleEntry> entries;
};

static Pass build(const std::vector<Bytes>& pats, uint32_t m)
{
    Pass p;
    p.m = m;
    p.pats = pats;
    p.filter.assign(sg::kSampleFilterWords, 0);
    p.heads.assign(sg::kSampleBuckets, 0);
    p.entries.resize(pats.size() * sg::kSampleStride);
    for (uint32_t j = 0; j < pats.size(); ++j) {
        uint8_t row[sg::kSampleRow];
        sg::sample_head_fill(row, pats[j].data(), m);
        for (uint32_t i = 0; i < sg::kSampleStride; ++i) {
            const uint32_t idx = j * sg::kSampleStride + i, gram = sg::sample_row_gram(row, i), h = sg::sample_hash(gram);
            p.filter[sg::sample_filter_word(h)] |= sg::sample_filter_bit(h);
            p.entries[idx] = sg::SampleEntry{gram, sg::sample_link(j, i, p.heads[sg::sample_bucket(h)])};
            p.heads[sg::sample_bucket(h)] = idx + 1;
        }
    }
    return p;
}

static std::vector<uint32_t> take_sample(const Bytes& padded, uint64_t n)
{
    std::vector<uint32_t> s(sg::sample_alloc_dwords(n), 0);
    for (uint64_t k = 0; k < sg::sample_count(n); ++k) std::memcpy(&s[k], padded.data() + k * sg::kSampleStride, 4);
    return s;
}

// the walk of [s_begin, s_end); passed / seen: samples that passed the filter / samples looked at
static std::vector<uint64_t> walk(const Pass& p, const Bytes& padded, const std::vector<uint32_t>& sample, uint64_t s_begin, uint64_t s_end,
                                  uint64_t* passed, uint64_t* seen)
{
    std::vector<uint64_t> counts(p.pats.size(), 0);
    if (s_end <= s_begin) return counts;
    for (uint64_t q = sg::sample_quad_first(s_begin); q < sg::sample_quad_end(s_end); ++q)
        for (uint32_t c = 0; c < 4; ++c) {
            const uint64_t k = 4 * q + c;
            const uint32_t gram = sample.at(k), h = sg::sample_hash(gram);
            ++*seen;
            if (!(p.filter[sg::sample_filter_word(h)] & sg::sample_filter_bit(h))) continue;
            ++*passed;
            for (uint32_t e = p.heads[sg::sample_bucket(h)]; e != 0;) {
                const sg::SampleEntry ent = p.entries.at(e - 1);
                e = sg::sample_link_next(ent.link);
                uint64_t s;
                if (ent.gram != gram || !sg::sample_window(k * sg::kSampleStride, sg::sample_link_offset(ent.link), s_begin, s_end, &s)) continue;
                const uint32_t j = sg::sample_link_pattern(ent.link);
                if (std::memcmp(padded.data() + s, p.pats[j].data(), p.m) == 0) ++counts[j];
            }
        }
    return counts;
}

static std::vector<uint64_t> brute(const std::vector<Bytes>& pats, uint32_t m, const Bytes& padded, uint64_t s_begin, uint64_t s_end)
{
    std::vector<uint64_t> counts(pats.size(), 0);
    for (uint32_t j = 0; j < pats.size(); ++j)
        for (uint64_t s = s_begin; s < s_end; ++s)
            if (std::memcmp(padded.data() + s, pats[j].data(), m) == 0) ++counts[j];
    return counts;
}

static int g_cases = 0, g_failures = 0;
static uint64_t g_passed = 0, g_seen = 0;

// one case: the pass over [s_begin, s_end) of text[0, n) against brute force
static void check(const char* what, const std::vector<Bytes>& pats, uint32_t m, const Bytes& text, uint64_t s_begin, uint64_t s_end)
{
    const uint64_t n = text.size();
    Bytes padded(text);
    padded.resize(n + kPad + sg::kSampleStride, 0);
    const std::vector<uint32_t> sample = take_sample(padded, n);
    const Pass p = build(pats, m);
    const std::vector<uint64_t> got = walk(p, padded, sample, s_begin, s_end, &g_passed, &g_seen), want = brute(pats, m, padded, s_begin, s_end);
    ++g_cases;
    if (got != want) {
        ++g_failures;
        for (uint32_t j = 0; j < pats.size(); ++j)
            if (got[j] != want[j]) { printf("FAIL %s m %u n %llu [%llu, %llu) pattern %u: %llu, brute force %llu\n", what, m, (unsigned long long)n, (unsigned long long)s_begin, (unsigned long long)s_end, j, (unsigned long long)got[j], (unsigned long long)want[j]); break; }
    }
}
static void check_whole(const char* what, const std::vector<Bytes>& pats, uint32_t m, const Bytes& text)
{
    check(what, pats, m, text, 0, text.size() >= m ? text.size() - m + 1 : 0);
}

static Bytes random_text(uint64_t n, uint32_t sigma, uint32_t base = 0)
{
    Bytes t(n);
    for (auto& b : t) b = (uint8_t)(base + rnd(sigma));
    return t;
}
static Bytes cut(const Bytes& t, uint64_t at, uint32_t m) { return Bytes(t.begin() + at, t.begin() + at + m); }
static void plant(Bytes& t, uint64_t at, const Bytes& p) { std::memcpy(t.data() + at, p.data(), p.size()); }

int main()
{
    const uint32_t ms[] = {31, 32, 33, 58, 59, 60, 64, 65, 66, 256};
    for (uint32_t m : ms) {
        // a pass of np patterns cut from 96 KiB of rand128, and the filter's pass rate (np: a by-value pass; at m = 32 also 152)
        for (uint32_t np : {sg::kSampleWidth, 152u}) {
            if (np == 152u && m != 32 && m != 64) continue;
            const uint64_t n = 96 << 10;
            Bytes t = random_text(n, 128);
            std::vector<Bytes> pats;
            for (uint32_t j = 0; j < np; ++j) pats.push_back(cut(t, rnd((uint32_t)(n - m)), m));
            // pattern 0 at every residue of s mod 28, at s = 0 and at s = n - m; pattern 1 twice in the pass
            for (uint32_t r = 0; r < sg::kSampleStride; ++r) plant(t, 2048 + (uint64_t)r * kStep + r, pats[0]);
            plant(t, 0, pats[0]);
            plant(t, n - m, pats[0]);
            pats[np - 1] = pats[1];
            g_passed = g_seen = 0;
            check_whole("rand128", pats, m, t);
            // the pass rate of a LARGE text is that of samples no pattern was cut from: 2 MiB of other rand128 (here a
            // sample in thirty lies inside a planted or cut copy)
            {
                const uint64_t n2 = 2 << 20;
                Bytes other = random_text(n2, 128);
                other.resize(n2 + kPad + sg::kSampleStride, 0);
                uint64_t passed = 0, seen = 0;
                (void)walk(build(pats, m), other, take_sample(other, n2), 0, n2 - m + 1, &passed, &seen);
                printf("rand128 m %3u np %3u: %.2f %% of the samples pass the filter (%.2f %% of this text's own)\n", m, np, 100.0 * (double)passed / (double)seen,
                       100.0 * (double)g_passed / (double)g_seen);
            }
            // sub-ranges whose ends are no multiples of 28 and that begin inside a gram
            check("sub-range", pats, m, t, 2048 + 1, 2048 + kStep * 3 + 2);
            check("sub-range", pats, m, t, 29, 30);
            check("sub-range", pats, m, t, 27, n - m);
            check("sub-range", pats, m, t, 2048 + 5 * kStep + 5, 2048 + 5 * kStep + 6);  // exactly the copy at residue 5
            check("sub-range", pats, m, t, 2048 + 5 * kStep + 6, 2048 + 9 * kStep);        // just behind it
        }
        // bytes of 128 and more
        {
            const uint64_t n = 32 << 10;
            Bytes t = random_text(n, 256);
            std::vector<Bytes> pats;
            for (uint32_t j = 0; j < 16; ++j) pats.push_back(cut(t, rnd((uint32_t)(n - m)), m));
            Bytes hi = random_text(m, 128, 128);
            pats.push_back(hi);
            for (uint32_t r = 0; r < 5; ++r) plant(t, 4096 + 997 * r, hi);
            check_whole("rand256", pats, m, t);
        }
        // the shortest texts: a pattern from the front and one from the back, over two symbols so that both may recur
        {
            std::vector<uint64_t> ns = {m, m + 1u, 55, 56, 57};
            for (uint32_t k = 2; k <= 11; ++k) { ns.push_back(28ull * k - 1); ns.push_back(28ull * k + 1); }
            for (uint64_t n : ns) {
                if (n < m) continue;
                const Bytes t = random_text(n, 2, 'a');
                check_whole("short text", {cut(t, 0, m), cut(t, n - m, m)}, m, t);
            }
        }
        // equal heads: two patterns whose first 31 bytes agree and that differ later; a pattern and its one-byte shift
        {
            const uint64_t n = 16 << 10;
            Bytes t = random_text(n, 128);
            std::vector<Bytes> pats;
            const Bytes a = cut(t, 1000, m);
            pats.push_back(a);
            if (m > sg::kSampleMinM) {
                Bytes b = a;
                b[m - 1] ^= 1;
                pats.push_back(b);
                for (uint32_t r = 0; r < 3; ++r) plant(t, 5000 + 613 * r, b);
            }
            pats.push_back(cut(t, 1001, m));  // the shift
            check_whole("equal heads, shift", pats, m, t);
        }
        // a periodic run of period 5 and a pattern from it: an occurrence every 5 bytes
        {
            const uint64_t n = 16 << 10;
            Bytes t = random_text(n, 128);
            for (uint64_t x = 3000; x < 3000 + 20 * (uint64_t)m; ++x) t[x] = (uint8_t)("abcab"[x % 5]);
            check_whole("period 5", {cut(t, 3005, m), cut(t, 3001, m), cut(t, 100, m)}, m, t);
        }
    }
    printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures != 0;
}
