// packed_host_check.cpp — what the packed-text calls decide on the host (smart_amd/csrc/planes_host.hpp), without a device:
// every bit of the planes encode_pattern and encode_sets write against the definition in planes.hpp, their counts and
// flags, order_spans on both of its paths, order_editl, and find_outcome over a small exhaustive grid.  Built and run by tests/test_packed_host.py under AddressSanitizer and UBSan;
// every buffer is a heap block of exactly the documented size.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "planes_host.hpp"

using sg::kPatWords;

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

static bool bit(const uint32_t* plane, uint32_t j) { return plane[j >> 5] >> (j & 31) & 1u; }

static const uint32_t kLengths[7] = {1, 31, 32, 33, 64, 65, SMARTGPU_XSIZE};

// encode_pattern: nvalues x m x {0, 1, several foreign bytes} x {without, with the SKIP plane}
static void pattern_cases()
{
    for (int nvalues = 1; nvalues <= 4; ++nvalues)
        for (uint32_t m : kLengths)
            for (int kind = 0; kind < 3; ++kind)
                for (int with_skip = 0; with_skip < 2; ++with_skip) {
                    uint8_t values[4] = {0, 0, 0, 0};  // ascending and distinct, none of them 255 (the foreign byte below)
                    for (int k = 0; k < nvalues; ++k) values[k] = (uint8_t)((k ? values[k - 1] + 1 : 0) + rnd(50));
                    std::vector<uint8_t> P(m);
                    std::vector<int> code(m);
                    for (uint32_t j = 0; j < m; ++j) {
                        code[j] = (int)rnd(nvalues);
                        P[j] = values[code[j]];
                    }
                    uint32_t want_foreign = 0;
                    for (int f = 0; f < (kind == 2 ? 5 : kind); ++f) {
                        const uint32_t j = f == 0 ? m - 1 : rnd(m);  // the last position among them
                        if (code[j] >= 0) ++want_foreign;
                        code[j] = -1;
                        P[j] = 255;
                    }
                    std::vector<uint32_t> X0(kPatWords, 0xA5A5A5A5u), X1(kPatWords, 0x5A5A5A5Au), SKIP(kPatWords, 0xFFFFFFFFu);
                    const uint32_t foreign = sg::encode_pattern(values, nvalues, P.data(), m, X0.data(), X1.data(), with_skip ? SKIP.data() : nullptr);
                    bool ok = foreign == want_foreign;
                    for (uint32_t j = 0; j < 32 * kPatWords; ++j) {
                        const int c = j < m ? code[j] : -1;
                        ok = ok && bit(X0.data(), j) == (c >= 0 && (c & 1)) && bit(X1.data(), j) == (c >= 0 && (c >> 1));
                        if (with_skip) ok = ok && bit(SKIP.data(), j) == (j < m && c < 0);
                    }
                    check(ok, "encode_pattern", nvalues, (int)m, kind, with_skip);
                }
}

// encode_sets: nvalues x m x {empty positions kept, filled} x {a mix with empty, full and singleton positions, all full,
// neither empty nor all full}; then a set that names a code the text does not hold, twice: the first is reported
static void set_cases()
{
    for (int nvalues = 1; nvalues <= 4; ++nvalues)
        for (uint32_t m : kLengths)
            for (int fill = 0; fill < 2; ++fill) {
                const uint32_t all = (1u << nvalues) - 1u;
                for (int kind = 0; kind < 3; ++kind) {
                    std::vector<uint8_t> sets(m);
                    for (uint32_t j = 0; j < m; ++j) sets[j] = (uint8_t)(kind == 1 ? all : kind == 2 ? 1 + rnd(all) : rnd(all + 1));
                    if (kind == 0) {
                        sets[rnd(m)] = (uint8_t)all;
                        sets[rnd(m)] = (uint8_t)(1u << rnd(nvalues));
                        sets[rnd(m)] = 0;
                    }
                    if (kind == 2 && all > 1) sets[rnd(m)] = 1;  // not full
                    uint32_t want_empty = 0;
                    bool want_full = true;
                    for (uint32_t j = 0; j < m; ++j) {
                        want_empty += sets[j] == 0;
                        want_full = want_full && sets[j] == all;
                    }
                    std::vector<uint32_t> Y(sg::kSetWords, 0xA5A5A5A5u);
                    uint32_t empty = 77;
                    bool full = !want_full;
                    bool ok = sg::encode_sets(nvalues, sets.data(), m, fill != 0, Y.data(), &empty, &full) == -1 && empty == want_empty && full == want_full;
                    for (uint32_t j = 0; j < 32 * kPatWords; ++j) {
                        uint32_t s = j < m ? sets[j] : 0;
                        if (j < m && (s == all || (s == 0 && fill))) s = 0xF;  // accepts everything, or counted by the host: all bits
                        for (uint32_t c = 0; c < 4; ++c) ok = ok && bit(Y.data() + c * kPatWords, j) == (s >> c & 1u);
                    }
                    check(ok, "encode_sets", nvalues, (int)m, fill, kind);
                }
                std::vector<uint8_t> sets(m);
                for (uint32_t j = 0; j < m; ++j) sets[j] = (uint8_t)rnd(all + 1);
                const uint32_t first = rnd(m), second = first + rnd(m - first);
                sets[second] = (uint8_t)(0x80u | rnd(16));
                sets[first] = (uint8_t)((1u << nvalues) | rnd(all + 1));
                std::vector<uint32_t> Y(sg::kSetWords);
                uint32_t empty = 0;
                bool full = false;
                check(sg::encode_sets(nvalues, sets.data(), m, fill != 0, Y.data(), &empty, &full) == (int)first, "encode_sets: bad set", nvalues, (int)m, fill,
                      (int)first);
            }
}

// Spans as planes_find writes them over the start positions [s_begin, s_last]: for every key a few ascending entries of
// span `key` (at least two), position << shift | a distance below 1 << shift.
typedef std::vector<std::vector<uint64_t>> Spans;
static Spans make_spans(const std::vector<uint64_t>& keys, uint64_t s_begin, uint64_t s_last, uint32_t shift)
{
    const uint64_t base = s_begin / 128 * 128;
    Spans spans;
    for (uint64_t key : keys) {
        const uint64_t lo = std::max(s_begin, base + key * sg::kFindSpan), hi = std::min(s_last, base + (key + 1) * sg::kFindSpan - 1);
        std::vector<uint64_t> span;
        uint64_t at = lo + rnd(100);
        for (uint32_t i = 0, cnt = 2 + rnd(4); i < cnt && at <= hi; ++i, at += 1 + rnd(1000)) span.push_back(at << shift | rnd(1u << shift));
        spans.push_back(span);
    }
    return spans;
}

static std::vector<uint64_t> flat(const Spans& spans)
{
    std::vector<uint64_t> v;
    for (const auto& s : spans) v.insert(v.end(), s.begin(), s.end());
    return v;
}

static void shuffle(Spans& spans)
{
    for (size_t i = spans.size() - 1; i > 0; --i) std::swap(spans[i], spans[rnd((uint32_t)i + 1)]);
    if (spans[0][0] < spans[1][0]) std::swap(spans[0], spans[1]);  // never left ascending
}

// order_spans: both paths x shift 0 and kMisShift x two ranges whose s_begin is no multiple of 128
static void span_cases()
{
    for (uint32_t shift : {0u, sg::kMisShift})
        for (uint64_t s_begin : {77ull, 1000003ull})
            for (int path = 0; path < 2; ++path) {
                // path 0, the table: 2000 spans of 3000; path 1, the sort: 6 spans of 16385, a range of more than 2^26 positions
                const uint64_t nkeys = path == 0 ? 3000 : 16385;
                const uint64_t s_last = s_begin / 128 * 128 + nkeys * sg::kFindSpan - 1 - rnd(1000);
                std::vector<uint64_t> keys;
                if (path == 0) {
                    for (uint64_t k = 0; k < nkeys; ++k)
                        if (k == 0 || k == nkeys - 1 || rnd(3)) keys.push_back(k);
                } else {
                    keys = {0, 1, 5000, 5001, 12000, nkeys - 1};
                }
                const bool path_ok = path == 0 ? nkeys <= 16 * keys.size() + 4096 && keys.size() > 1500 : nkeys > 16 * (keys.size() + 1) + 4096 && s_last - s_begin > (1ull << 26);
                const Spans sorted = make_spans(keys, s_begin, s_last, shift);
                const std::vector<uint64_t> want = flat(sorted);
                bool ascending = path_ok;
                for (size_t i = 1; i < want.size(); ++i) ascending = ascending && want[i - 1] < want[i];
                check(ascending, "order_spans: the case itself", (int)shift, (int)s_begin, path, 0);

                std::vector<uint64_t> v = want;  // already ascending: left in place
                check(sg::order_spans(v.data(), v.size(), s_begin, s_last, shift) && v == want, "order_spans: ascending", (int)shift, (int)s_begin, path, 0);
                check(sg::order_spans(v.data(), 0, s_begin, s_last, shift) && v == want, "order_spans: no entry", (int)shift, (int)s_begin, path, 0);

                Spans mixed = sorted;  // span order shuffled
                shuffle(mixed);
                v = flat(mixed);
                check(v != want && sg::order_spans(v.data(), v.size(), s_begin, s_last, shift) && v == want, "order_spans: shuffled", (int)shift, (int)s_begin, path, 0);

                Spans split = mixed;  // a span in two pieces, others between them
                split.push_back(std::vector<uint64_t>(1, split[0].back()));
                split[0].pop_back();
                v = flat(split);
                check(!sg::order_spans(v.data(), v.size(), s_begin, s_last, shift), "order_spans: a span in two pieces", (int)shift, (int)s_begin, path, 0);

                Spans swapped = mixed;  // a non-ascending pair inside a span
                std::swap(swapped[2][0], swapped[2][1]);
                v = flat(swapped);
                check(!sg::order_spans(v.data(), v.size(), s_begin, s_last, shift), "order_spans: a descending pair", (int)shift, (int)s_begin, path, 0);
                swapped = mixed;  // and an equal one
                swapped[2][1] = swapped[2][0];
                v = flat(swapped);
                check(!sg::order_spans(v.data(), v.size(), s_begin, s_last, shift), "order_spans: an equal pair", (int)shift, (int)s_begin, path, 0);

                if (path == 1) continue;  // the table path alone knows the number of spans of the range
                for (int side = 0; side < 2; ++side) {  // a key outside the range: beyond its last span, before its first
                    Spans outside = mixed;
                    const uint64_t far = side == 0 ? s_begin / 128 * 128 + nkeys * sg::kFindSpan + 5 : s_begin / 128 * 128 - 1;
                    outside.insert(outside.begin() + 1, std::vector<uint64_t>(1, far << shift));
                    v = flat(outside);
                    check(!sg::order_spans(v.data(), v.size(), s_begin, s_last, shift), "order_spans: a key outside the range", (int)shift, (int)s_begin, path, side);
                }
            }
}

// find_outcome: what a cursor means, over bound x cap x room_got x total.  The expected letters are written out by hand from
// the four cases (B: cursor beyond the bound; C: list complete; O: more than cap; N: fits cap, the device had no room), one
// letter per total = 0 .. bound + 1; the rows stand in the order the grid produces them, duplicates included.
struct OutcomeRow { uint64_t bound, cap, room_got; const char* want; };
static const OutcomeRow kOutcomes[] = {
    // bound 1: cap 0, 1, bound - 1, bound, bound + 1; room_got 0, min(cap, bound)
    {1, 0, 0, "COB"}, {1, 0, 0, "COB"},
    {1, 1, 0, "CNB"}, {1, 1, 1, "CCB"},
    {1, 0, 0, "COB"}, {1, 0, 0, "COB"},
    {1, 1, 0, "CNB"}, {1, 1, 1, "CCB"},
    {1, 2, 0, "CNB"}, {1, 2, 1, "CCB"},
    // bound 5
    {5, 0, 0, "COOOOOB"}, {5, 0, 0, "COOOOOB"},
    {5, 1, 0, "CNOOOOB"}, {5, 1, 1, "CCOOOOB"},
    {5, 4, 0, "CNNNNOB"}, {5, 4, 4, "CCCCCOB"},
    {5, 5, 0, "CNNNNNB"}, {5, 5, 5, "CCCCCCB"},
    {5, 6, 0, "CNNNNNB"}, {5, 6, 5, "CCCCCCB"},
};

static char outcome_letter(sg::FindOutcome o)
{
    switch (o) {
    case sg::FindOutcome::kBeyondBound: return 'B';
    case sg::FindOutcome::kComplete: return 'C';
    case sg::FindOutcome::kOverCap: return 'O';
    case sg::FindOutcome::kNoRoom: return 'N';
    }
    return '?';
}

static void outcome_cases()
{
    size_t row = 0;
    for (uint64_t bound : {uint64_t(1), uint64_t(5)})
        for (uint64_t cap : {uint64_t(0), uint64_t(1), bound - 1, bound, bound + 1})
            for (uint64_t room_got : {uint64_t(0), std::min(cap, bound)}) {
                const OutcomeRow& r = kOutcomes[row++];
                const bool row_ok = r.bound == bound && r.cap == cap && r.room_got == room_got;  // the table follows the grid
                for (uint64_t total = 0; total <= bound + 1; ++total)
                    check(row_ok && outcome_letter(sg::find_outcome(total, bound, room_got, cap)) == r.want[total], "find_outcome", (int)bound, (int)cap,
                          (int)room_got, (int)total);
            }
}

// order_editl: entries (e << shift) | distance over the end positions [lo, hi] with distances <= k
static void editl_cases()
{
    const uint32_t shift = 5, k = 9;
    const uint64_t lo = 129, hi = 100000;
    std::vector<uint64_t> want;
    for (uint64_t e = lo; e < hi; e += 1 + rnd(700)) want.push_back(e << shift | rnd(k + 1));
    want.push_back(hi << shift | k);  // both ends of the range, the largest distance
    want[0] = lo << shift;

    std::vector<uint64_t> v = want;
    check(sg::order_editl(v.data(), v.size(), lo, hi, k, shift) && v == want, "order_editl: sorted", 0, 0, 0, 0);
    for (size_t i = v.size() - 1; i > 0; --i) std::swap(v[i], v[rnd((uint32_t)i + 1)]);
    std::swap(v[0], v[1]);
    check(v != want && sg::order_editl(v.data(), v.size(), lo, hi, k, shift) && v == want, "order_editl: shuffled", 0, 0, 0, 0);
    const std::vector<uint64_t> untouched = {want[3], want[1], want[2]};
    v = untouched;
    check(sg::order_editl(v.data(), 0, lo, hi, k, shift) && v == untouched, "order_editl: no entry", 0, 0, 0, 0);

    const uint64_t bad[4] = {
        (want[5] >> shift) << shift | ((want[5] & 31) ^ 1),  // an end position twice, with another distance
        (lo - 1) << shift,                                    // an end below lo
        (hi + 1) << shift,                                    // an end above hi
        (lo + 1) << shift | (k + 1),                          // a distance of k + 1
    };
    for (int b = 0; b < 4; ++b) {
        v = want;
        if (b == 3) v[1] = bad[b]; else v.insert(v.begin() + 2, bad[b]);
        check(!sg::order_editl(v.data(), v.size(), lo, hi, k, shift), "order_editl: refused", b, 0, 0, 0);
    }
}

int main()
{
    pattern_cases();
    set_cases();
    span_cases();
    outcome_cases();
    editl_cases();
    printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
