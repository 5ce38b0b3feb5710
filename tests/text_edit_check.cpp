// text_edit_check.cpp — the host side of the edit-distance calls on BYTE texts on the CPU (tests/test_text_edit.py builds
// it with AddressSanitizer and UBSan and runs it): the 256 masks of smart_amd/csrc/tedit_host.hpp bit by bit, the run
// geometry edit_run_walk against a scalar model that only counts and compares, and a CPU emulation of "every lane walks its
// run from a fresh start" (edit_run_walk, the masks' table, edit_step) against the full DP on the range.
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
#include "edit_step.hpp"
#include "tedit_host.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace {

int g_cases = 0, g_failures = 0;

void check(bool ok, const char* what, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0)
{
    ++g_cases;
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s (%llu, %llu, %llu)\n", what, a, b, c);
}

unsigned long long g_x = 88172645463325252ull;
unsigned rnd(unsigned mod)
{
    g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17;
    return static_cast<unsigned>((g_x >> 11) % mod);
}

bool row_bit(const std::vector<uint8_t>& classes, uint32_t j, uint32_t v) { return classes[32 * j + v / 8] >> (v % 8) & 1; }

// every bit of peq against `accepts(j, v)`, and zero from m on
template <typename F>
bool peq_is(const uint32_t (&peq)[256][sg::kTEditWords], uint32_t m, F accepts)
{
    for (uint32_t v = 0; v < 256; ++v)
        for (uint32_t j = 0; j < 32 * sg::kTEditWords; ++j) {
            const bool have = peq[v][j / 32] >> (j % 32) & 1, want = j < m && accepts(j, v);
            if (have != want) return false;
        }
    return true;
}

// ---- the masks: 5 lengths x 3 checks -----------------------------------------------------------------------------------
void check_masks()
{
    for (uint32_t m : {1u, 31u, 32u, 33u, 64u}) {
        // a byte pattern with the bytes 0 and 255 and one byte repeated (m = 1: byte 255 alone)
        std::vector<uint8_t> P(m);
        for (uint32_t j = 0; j < m; ++j) P[j] = static_cast<uint8_t>(rnd(256));
        P[m - 1] = 255;
        if (m > 1) P[0] = 0;
        if (m > 3) P[1] = P[m - 2] = 'e';
        uint32_t peq[256][sg::kTEditWords];
        std::fill(&peq[0][0], &peq[0][0] + 256 * sg::kTEditWords, 0xDEADBEEFu);
        sg::edit_peq_bytes(P.data(), m, peq);
        check(peq_is(peq, m, [&](uint32_t j, uint32_t v) { return P[j] == v; }), "edit_peq_bytes", m);
        // the same pattern as rows of one bit
        std::vector<uint8_t> one(32 * m, 0);
        for (uint32_t j = 0; j < m; ++j) one[32 * j + P[j] / 8] |= static_cast<uint8_t>(1u << (P[j] % 8));
        uint32_t peq1[256][sg::kTEditWords];
        std::fill(&peq1[0][0], &peq1[0][0] + 256 * sg::kTEditWords, 0xDEADBEEFu);
        sg::edit_peq_classes(one.data(), m, peq1);
        check(std::equal(&peq[0][0], &peq[0][0] + 256 * sg::kTEditWords, &peq1[0][0]), "edit_peq_classes of singletons", m);
        // random rows, an empty row and a full row
        std::vector<uint8_t> rows(32 * m);
        for (auto& b : rows) b = static_cast<uint8_t>(rnd(256));
        const uint32_t full = m - 1, empty = m > 1 ? m / 2 - (m / 2 == full) : m;  // (m = 1: the full row only)
        for (uint32_t i = 0; i < 32; ++i) {
            rows[32 * full + i] = 0xFF;
            if (empty < m) rows[32 * empty + i] = 0;
        }
        sg::edit_peq_classes(rows.data(), m, peq1);
        check(peq_is(peq1, m, [&](uint32_t j, uint32_t v) { return row_bit(rows, j, v); }), "edit_peq_classes", m);
    }
}

// ---- the geometry: 7 range starts x 7 range ends x 2 warm-ups ---------------------------------------------------------------
// The scalar model knows no arithmetic of runs: it visits the 128 positions of run c one by one, keeps those of the range,
// and steps back from the first of them, one byte at a time, at most mk times and never below e_begin.
sg::EditWalk model_walk(uint64_t c, uint64_t e_begin, uint64_t e_end, uint32_t mk)
{
    bool any = false;
    uint64_t lo = 0, hi = 0;
    for (uint64_t p = c * 128; p < c * 128 + 128; ++p) {
        if (p < e_begin || p >= e_end) continue;
        if (!any) lo = p;
        any = true;
        hi = p + 1;
    }
    sg::EditWalk w = {0, 0, 0};
    if (!any) return w;
    uint64_t start = lo;
    for (uint32_t i = 0; i < mk && start > e_begin; ++i) --start;
    w.first = static_cast<int>(static_cast<long long>(start) - static_cast<long long>(c * 128));
    w.own = static_cast<int>(lo - c * 128);
    w.last = static_cast<int>(hi - c * 128);
    return w;
}

void check_geometry()
{
    // e_begin: text byte 0; a run's first byte, a byte in its middle, its last byte; either side of a wave's span and mid-run behind it
    const uint64_t begins[7] = {0, 128, 200, 255, 8191, 8192, 8200};
    // e_end: one byte behind e_begin; one before, at and one after a multiple of 128 (65 * 128) and of 8192
    const long long ends[7] = {-1, 8320 - 1, 8320, 8320 + 1, 16384 - 1, 16384, 16384 + 1};
    for (uint64_t e_begin : begins)
        for (long long e : ends)
            for (uint32_t mk : {1u, 71u}) {
                const uint64_t e_end = e < 0 ? e_begin + 1 : static_cast<uint64_t>(e);
                bool ok = e_end > e_begin;
                uint64_t owned = 0;
                // every run from the one before the range (run 0: none) to two behind it: those at both ends, those outside
                for (uint64_t c = e_begin / 128 ? e_begin / 128 - 1 : 0; c <= e_end / 128 + 2; ++c) {
                    const sg::EditWalk w = sg::edit_run_walk(c, e_begin, e_end, mk), want = model_walk(c, e_begin, e_end, mk);
                    ok = ok && w.first == want.first && w.own == want.own && w.last == want.last;
                    // what the kernels rely on: the warm-up is at most mk bytes of the row before, owned bytes lie in the run
                    ok = ok && w.first >= -static_cast<int>(mk) && w.first <= w.own && w.own == std::max(w.first, 0) && w.own <= w.last && w.last <= 128;
                    ok = ok && static_cast<long long>(c * 128) + w.first >= static_cast<long long>(w.last > w.own ? e_begin : 0);
                    owned += static_cast<uint64_t>(w.last - w.own);
                }
                check(ok && owned == e_end - e_begin, "edit_run_walk", e_begin, e_end, mk);
            }
}

// ---- the walk: 2 texts x 2 lengths x 3 k x 2 ranges ---------------------------------------------------------------------
// the last row of Sellers' DP over T[from, to): D[0][*] = 0, the column before `from` is D[i] = i
std::vector<int> dp_scores(const std::vector<uint8_t>& P, const std::vector<uint8_t>& T, size_t from, size_t to)
{
    const size_t m = P.size();
    std::vector<int> col(m + 1), next(m + 1), out;
    for (size_t i = 0; i <= m; ++i) col[i] = static_cast<int>(i);
    for (size_t e = from; e < to; ++e) {
        next[0] = 0;
        for (size_t i = 1; i <= m; ++i) next[i] = std::min(col[i - 1] + (P[i - 1] != T[e]), std::min(col[i] + 1, next[i - 1] + 1));
        col.swap(next);
        out.push_back(col[m]);
    }
    return out;
}

// what the kernels compute: every run's lane starts fresh at edit_run_walk's first byte, reads its masks from the table and
// keeps the scores of the bytes it owns
template <int WORDS>
std::vector<int> lane_scores(const std::vector<uint8_t>& P, uint32_t k, const std::vector<uint8_t>& T, uint64_t from, uint64_t to)
{
    const uint32_t m = static_cast<uint32_t>(P.size());
    uint32_t peq[256][sg::kTEditWords];
    sg::edit_peq_bytes(P.data(), m, peq);
    std::vector<uint32_t> table(256 * WORDS);
    sg::edit_peq_table(peq, WORDS, table.data());
    std::vector<int> out(to - from, -1);
    for (uint64_t c = from / 128; c * 128 < to; ++c) {
        const sg::EditWalk w = sg::edit_run_walk(c, from, to, m + k);
        uint32_t pv[WORDS], mv[WORDS];
        sg::edit_fresh<WORDS>(pv, mv);
        int score = static_cast<int>(m);
        for (int p = w.first; p < w.last; ++p) {
            const uint64_t at = c * 128 + static_cast<uint64_t>(static_cast<long long>(p));
            uint32_t eq[WORDS];
            for (int i = 0; i < WORDS; ++i) eq[i] = table[T.at(at) * WORDS + i];
            score += sg::edit_step<WORDS>(pv, mv, eq, m - 1);
            if (p >= w.own) out.at(at - from) = score;
        }
    }
    return out;
}

void check_walk()
{
    const size_t n = 40 * 1024;
    for (unsigned values : {256u, 2u})
        for (uint32_t m : {20u, 64u})
            for (uint32_t k : {0u, 3u, 7u}) {
                std::vector<uint8_t> T(n);
                for (auto& b : T) b = static_cast<uint8_t>(values == 2 ? (rnd(2) ? 'a' : 'b') : rnd(256));
                std::vector<uint8_t> P(T.begin() + 5000, T.begin() + 5000 + m);
                // copies of the pattern with up to k + 1 edits that end around the seams of a lane's run and a wave's span
                for (size_t end : {128u * 9 - 1, 128u * 17, 128u * 25 + 1, 8192u - 1, 8192u, 8193u, 16384u + 40, 3u * 8192 + 127}) {
                    std::vector<uint8_t> Q = P;
                    for (uint32_t e = rnd(k + 2); e > 0 && Q.size() > 1; --e) {
                        const size_t at = rnd(static_cast<unsigned>(Q.size()));
                        const unsigned kind = rnd(3);
                        if (kind == 0) Q[at] = static_cast<uint8_t>(Q[at] + 1);
                        else if (kind == 1) Q.erase(Q.begin() + static_cast<long>(at));
                        else Q.insert(Q.begin() + static_cast<long>(at), static_cast<uint8_t>(values == 2 ? 'a' : rnd(256)));
                    }
                    std::copy(Q.begin(), Q.end(), T.begin() + static_cast<long>(end + 1 - Q.size()));
                }
                for (int range = 0; range < 2; ++range) {
                    // the whole text; a range that begins and ends mid-run, its first copy cut by the range's start
                    const uint64_t from = range ? 128 * 9 - 10 : 0, to = range ? n - 777 : n;
                    const std::vector<int> want = dp_scores(P, T, from, to);
                    const std::vector<int> got = m <= 32 ? lane_scores<1>(P, k, T, from, to) : lane_scores<2>(P, k, T, from, to);
                    bool ok = got.size() == want.size();
                    uint64_t bad = 0, hits = 0;
                    for (size_t i = 0; ok && i < want.size(); ++i) {
                        // every value <= k is equal, every value > k is > k
                        const bool same = want[i] <= static_cast<int>(k) ? got[i] == want[i] : got[i] > static_cast<int>(k);
                        hits += want[i] <= static_cast<int>(k);
                        if (!same) { ok = false; bad = from + i; }
                    }
                    check(ok && hits > 0, "lanes from fresh starts against the full DP", values * 1000 + m, k, bad);
                }
            }
}

}  // namespace

int main()
{
    check_masks();
    check_geometry();
    check_walk();
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
