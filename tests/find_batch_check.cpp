// find_batch_check.cpp — smartgpu_find_batch64 without a device (tests/test_find_batch.py compiles and runs this, plain
// and under AddressSanitizer / UBSan).
//  1. order_find_batch (multi_find_host.hpp) over shuffled entries of a naive search: the slices, and every refusal.
//  2. A CPU model of hor_multi_find's walk (k_hormf.hip): the table of multi.hpp built from the staged rows, per tile and
//     per lane the skip walk over the lane's 64 window ends with the back halo, the chains, the compare in "LDS" and
//     its completion in "memory", the stage with its overflow path and the flush — several passes on one cursor.  It
//     must emit exactly the naive (s, k) set, and its two tallies must agree.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "multi_find.hpp"
#include "multi_find_host.hpp"

using namespace sg;

static int g_cases = 0, g_failures = 0;
static void check(bool ok, const char* what, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0)
{
    ++g_cases;
    if (!ok) {
        ++g_failures;
        std::printf("FAIL %s (%u, %u, %u)\n", what, a, b, c);
    }
}

typedef std::vector<std::vector<uint8_t>> Patterns;

static std::vector<std::vector<uint64_t>> naive(const std::vector<uint8_t>& T, uint64_t off, uint64_t n, const Patterns& P)
{
    std::vector<std::vector<uint64_t>> r(P.size());
    for (size_t k = 0; k < P.size(); ++k) {
        const size_t m = P[k].size();
        for (uint64_t s = off; m <= n && s + m <= off + n; ++s)
            if (std::memcmp(T.data() + s, P[k].data(), m) == 0) r[k].push_back(s);
    }
    return r;
}

// ---- 1. order_find_batch ---------------------------------------------------------------------------------------------
static void order_cases()
{
    std::mt19937_64 rng(0xF1DBA7C4u);
    std::vector<uint8_t> T(5000);
    for (auto& b : T) b = (uint8_t)(rng() % 3);
    const uint64_t off = 17, n = 4900;
    const uint32_t m = 4;
    Patterns P;
    for (uint32_t k = 0; k < 9; ++k) P.push_back(std::vector<uint8_t>(T.begin() + 100 * k + 20, T.begin() + 100 * k + 20 + m));
    P[4] = P[1];                        // the same pattern twice
    P[6] = {9, 9, 9, 9};                // an empty slice
    P[8] = {9, 9, 9, 8};                // and one at the end
    const uint32_t K = (uint32_t)P.size();
    const auto want = naive(T, off, n, P);
    std::vector<uint64_t> counts(K), entries;
    for (uint32_t k = 0; k < K; ++k) {
        counts[k] = want[k].size();
        for (uint64_t s : want[k]) entries.push_back((s << kFindBatchShift) | k);
    }
    std::shuffle(entries.begin(), entries.end(), rng);
    const uint64_t total = entries.size(), lo = off, hi = off + n - m;
    {
        std::vector<uint64_t> e = entries, starts(K + 1, 77);
        bool ok = order_find_batch(e.data(), total, K, counts.data(), lo, hi, starts.data());
        for (uint32_t k = 0; ok && k < K; ++k)
            ok = starts[k + 1] - starts[k] == want[k].size() && std::equal(want[k].begin(), want[k].end(), e.begin() + starts[k]);
        check(ok && starts[0] == 0 && starts[K] == total && want[4] == want[1] && !want[1].empty() && want[6].empty(), "order: shuffled entries come back as the naive slices");
    }
    {   // nothing at all
        std::vector<uint64_t> zero(K, 0), starts(K + 1, 77);
        check(order_find_batch(nullptr, 0, K, zero.data(), lo, hi, starts.data()) && starts[K] == 0, "order: an empty list");
    }
    std::vector<uint64_t> starts(K + 1);
    {   // an index >= K
        std::vector<uint64_t> e = entries;
        e[total / 2] = (e[total / 2] & ~((1ull << kFindBatchShift) - 1)) | K;
        check(!order_find_batch(e.data(), total, K, counts.data(), lo, hi, starts.data()), "order: an index >= K is refused");
    }
    {   // a position below lo, and one above hi
        std::vector<uint64_t> e = entries;
        e[3] = ((lo - 1) << kFindBatchShift) | (e[3] & ((1ull << kFindBatchShift) - 1));
        check(!order_find_batch(e.data(), total, K, counts.data(), lo, hi, starts.data()), "order: a position below the range is refused");
        e = entries;
        e[3] = ((hi + 1) << kFindBatchShift) | (e[3] & ((1ull << kFindBatchShift) - 1));
        check(!order_find_batch(e.data(), total, K, counts.data(), lo, hi, starts.data()), "order: a position above the range is refused");
    }
    {   // a tally that differs from its count: an entry of pattern 0 relabelled as pattern 2 (the total still agrees)
        std::vector<uint64_t> e = entries;
        for (auto& x : e)
            if ((x & ((1ull << kFindBatchShift) - 1)) == 0) { x |= 2; break; }
        check(!order_find_batch(e.data(), total, K, counts.data(), lo, hi, starts.data()), "order: a tally that differs from its count is refused");
        std::vector<uint64_t> c = counts;  // and counts that do not add up to the total
        ++c[6];
        e = entries;
        check(!order_find_batch(e.data(), total, K, c.data(), lo, hi, starts.data()), "order: counts that are not the total are refused");
    }
    {   // a position twice in one slice (the tallies agree)
        std::vector<uint64_t> e = entries;
        size_t first = total, second = total;
        for (size_t i = 0; i < total; ++i)
            if ((e[i] & ((1ull << kFindBatchShift) - 1)) == 1) { (first == total ? first : second) = i; if (second != total) break; }
        e[second] = e[first];
        check(second != total && !order_find_batch(e.data(), total, K, counts.data(), lo, hi, starts.data()), "order: a duplicate position is refused");
    }
}

// ---- 2. the kernel's walk ----------------------------------------------------------------------------------------------
struct Model {
    static constexpr uint32_t kThreads = 256, kL = 64, kTB = kThreads * kL;
    const std::vector<uint8_t>& T;
    uint32_t stage_cap;
    std::vector<std::pair<uint64_t, uint32_t>> out;  // what reached the output: (s, index)
    uint64_t cursor = 0;
    std::vector<uint64_t> counts;
    bool in_bounds = true;  // every read stayed inside what the kernel has in LDS

    Model(const std::vector<uint8_t>& text, uint32_t K, uint32_t stage) : T(text), stage_cap(stage), counts(K, 0) {}

    // one pass: patterns base .. base + np - 1 of P over the start positions [s_begin, s_end)
    void pass(const Patterns& P, uint32_t base, uint32_t np, uint64_t s_begin, uint64_t s_end)
    {
        const uint32_t m = (uint32_t)P[base].size(), H = m - 1 < kHaloMaxFind ? m - 1 : kHaloMaxFind, H16 = (H + 15u) & ~15u;
        const uint32_t stride = tail_stride(m), rlast = m - 1 - gram_first(m);
        // the staged rows, and the table, heads and links built from them as the prologue does
        std::vector<uint8_t> rows((size_t)np * stride);
        for (uint32_t g = 0; g < np; ++g) {
            uint8_t row[kTailRow];
            tail_fill(row, P[base + g].data(), m);
            std::memcpy(rows.data() + (size_t)g * stride, row, stride);
        }
        std::vector<uint8_t> gram(kGramSlots, (uint8_t)gram_default(m));
        std::vector<uint32_t> heads(kGramBuckets, 0), next(np, 0), sums(np, 0);
        for (uint32_t g = 0; g < np; ++g)
            for (uint32_t i = gram_first(m); i + 3 <= m; ++i) {
                const uint32_t two = tail_gram_at(rows.data() + (size_t)g * stride, m, i);
                uint8_t& b = gram[gram_slot(two & 0xFFu, two >> 8)];
                if (b > gram_shift(m, i)) b = (uint8_t)gram_shift(m, i);
            }
        for (uint32_t g = 0; g < np; ++g) {
            const uint32_t two = tail_gram_at(rows.data() + (size_t)g * stride, m, m - 2);
            gram[gram_slot(two & 0xFFu, two >> 8)] |= kGramHit;
            const uint32_t bucket = gram_bucket(two & 0xFFu, two >> 8);
            next[g] = heads[bucket];
            heads[bucket] = g + 1;
        }
        const uint64_t e_begin = s_begin + m - 1, e_end = s_end + m - 1;
        if (e_end <= e_begin) return;
        std::vector<std::pair<uint64_t, uint32_t>> stage;
        uint32_t taken = 0;
        auto emit = [&](uint32_t g, uint64_t s) {
            ++sums[g];
            if (taken++ < stage_cap) stage.push_back({s, base + g});
            else { ++cursor; out.push_back({s, base + g}); }  // the stage is full: straight behind the cursor
        };
        auto flush = [&]() {
            cursor += stage.size();
            out.insert(out.end(), stage.begin(), stage.end());
            stage.clear();
            taken = 0;
        };
        for (uint64_t t = e_begin / kTB; t <= (e_end - 1) / kTB; ++t) {
            const uint64_t tile0 = t * kTB;
            flush();
            // what the tile holds: T[tile0 - H16, tile0 + kTB) (the pads of a device text are zero)
            auto lds = [&](uint32_t i) -> uint32_t {  // i in tile coordinates: txt[H16 + x] == T[tile0 + x]
                if (i >= H16 + kTB) { in_bounds = false; return 0; }
                const int64_t at = (int64_t)tile0 + (int64_t)i - (int64_t)H16;
                return at < 0 || at >= (int64_t)T.size() ? 0u : T[(size_t)at];
            };
            for (uint32_t lane = 0; lane < kThreads; ++lane) {
                const uint64_t seg = tile0 + (uint64_t)lane * kL;
                const uint64_t lo = seg > e_begin ? seg : e_begin, hi = seg + kL < e_end ? seg + kL : e_end;
                if (lo >= hi) continue;
                const uint32_t e0 = (uint32_t)(lo - tile0) + H16, ehi = (uint32_t)(hi - tile0) + H16;
                bool parked = false;
                uint32_t parked_g = 0;
                uint64_t parked_s = 0;
                auto rest_equal = [&](uint32_t g, uint64_t s) { return std::memcmp(T.data() + s, P[base + g].data(), m - 1 - H) == 0; };
                for (uint32_t e = e0; e < ehi;) {
                    if (e < 1) { in_bounds = false; break; }
                    const uint32_t prev = lds(e - 1), last = lds(e);
                    const uint32_t ent = gram[gram_slot(prev, last)];
                    if (gram_byte_hit(ent))
                        for (uint32_t c = heads[gram_bucket(prev, last)]; c != 0; c = next[c - 1]) {
                            const uint32_t g = c - 1;
                            const uint8_t* prow = rows.data() + (size_t)g * stride;
                            uint32_t k = 0;
                            while (k <= H && e >= k && prow[rlast - k] == lds(e - k)) ++k;
                            bool ok = k == H + 1;
                            const uint64_t s = tile0 + (e - H16) - (m - 1);
                            if (m - 1 > H && ok) {
                                if (!parked) { parked = true; parked_g = g; parked_s = s; ok = false; }
                                else ok = rest_equal(g, s);
                            }
                            if (ok) emit(g, s);
                        }
                    if (gram_byte_shift(ent) == 0) { in_bounds = false; break; }  // a walk that does not move
                    e += gram_byte_shift(ent);
                }
                if (parked && rest_equal(parked_g, parked_s)) emit(parked_g, parked_s);
            }
        }
        flush();
        for (uint32_t g = 0; g < np; ++g) counts[base + g] += sums[g];
    }
};

static void walk_case(const std::vector<uint8_t>& T, uint32_t text_id, uint32_t m, uint32_t stage_cap, std::mt19937_64& rng)
{
    const uint64_t off = 129, n = T.size() - off - 77;
    Patterns P;
    const uint64_t cuts[] = {off, off + 1, 16384 - m + 1, 16384, 16385 - m, 2 * 16384 - m / 2, off + n - m, 20000, 63, 64 * 7 + 1};
    for (uint64_t c : cuts) P.push_back(std::vector<uint8_t>(T.begin() + c, T.begin() + c + m));
    P.push_back(P[3]);  // the same pattern twice
    P.push_back(std::vector<uint8_t>(T.begin() + off - 1, T.begin() + off - 1 + m));  // begins before the range
    std::vector<uint8_t> absent(m);
    for (auto& b : absent) b = (uint8_t)(rng() | 1);
    absent[m - 1] = 0xFE;
    P.push_back(absent);
    const uint32_t K = (uint32_t)P.size();
    Model model(T, K, stage_cap);
    const uint32_t width = 5;  // three passes on one cursor
    for (uint32_t base = 0; base < K; base += width) model.pass(P, base, K - base < width ? K - base : width, off, off + n - m + 1);
    const auto want = naive(T, off, n, P);
    std::set<std::pair<uint64_t, uint32_t>> want_set, got_set(model.out.begin(), model.out.end());
    uint64_t total = 0;
    bool counts_ok = true;
    for (uint32_t k = 0; k < K; ++k) {
        for (uint64_t s : want[k]) want_set.insert({s, k});
        total += want[k].size();
        counts_ok = counts_ok && model.counts[k] == want[k].size();
    }
    check(model.in_bounds && got_set == want_set && model.out.size() == total && model.cursor == total && counts_ok && total >= 10,
          "walk: the model emits the naive (s, k) set", text_id, m, stage_cap);
}

int main()
{
    order_cases();
    std::mt19937_64 rng(0x5EEDF1DDu);
    const uint32_t sigmas[] = {2, 128, 256, 1};
    for (uint32_t ti = 0; ti < 4; ++ti) {
        std::vector<uint8_t> T(2 * 16384 + 300 + 129 + 77);
        for (auto& b : T) b = sigmas[ti] == 1 ? (uint8_t)0xA7 : (uint8_t)(rng() % sigmas[ti]);
        for (uint32_t m : {3u, 4u, 16u, 17u, 18u, 33u, 65u, 300u})
            for (uint32_t stage_cap : {1u, 4u}) walk_case(T, ti, m, stage_cap, rng);
    }
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
