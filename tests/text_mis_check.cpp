// text_mis_check.cpp — the host side of the mismatch calls on BYTE texts on the CPU (tests/test_text_mis.py builds it with
// AddressSanitizer and UBSan and runs it): the 256 masks "position j does not accept this byte" of
// smart_amd/csrc/tmis_host.hpp bit by bit, and a CPU emulation of "every lane walks its run from a fresh start m - 1 bytes
// before it" (edit_run_walk, the masks' table, mis_step, mis_hit, mis_raw) and of the walk as the kernels take it (from
// mis_walk_start, whole dwords, answers kept by mis_keep_from / mis_group_mask) against the definition as a triple loop —
// every range, every start of the range, every pattern position.
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
#include "tmis_host.hpp"

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

const uint32_t kLengths[7] = {1, 2, 31, 32, 33, 63, 64};

bool row_bit(const std::vector<uint8_t>& classes, uint32_t j, uint32_t v) { return classes[32 * j + v / 8] >> (v % 8) & 1; }

// every bit of neq against `accepts(j, v)`: set below m where position j does NOT accept v, zero from m on
template <typename F>
bool neq_is(const uint32_t (&neq)[256][sg::kTEditWords], uint32_t m, F accepts)
{
    for (uint32_t v = 0; v < 256; ++v)
        for (uint32_t j = 0; j < 32 * sg::kTEditWords; ++j) {
            const bool have = neq[v][j / 32] >> (j % 32) & 1, want = j < m && !accepts(j, v);
            if (have != want) return false;
        }
    return true;
}

// ---- the masks: 7 lengths x 3 checks -----------------------------------------------------------------------------------
void check_masks()
{
    for (uint32_t m : kLengths) {
        // a byte pattern with the bytes 0 and 255 and one byte repeated (m = 1: byte 255 alone)
        std::vector<uint8_t> P(m);
        for (uint32_t j = 0; j < m; ++j) P[j] = static_cast<uint8_t>(rnd(256));
        P[m - 1] = 255;
        if (m > 1) P[0] = 0;
        if (m > 3) P[1] = P[m - 2] = 'e';
        uint32_t neq[256][sg::kTEditWords];
        std::fill(&neq[0][0], &neq[0][0] + 256 * sg::kTEditWords, 0xDEADBEEFu);
        sg::mis_neq_bytes(P.data(), m, neq);
        check(neq_is(neq, m, [&](uint32_t j, uint32_t v) { return P[j] == v; }), "mis_neq_bytes", m);
        // the same pattern as rows of one bit
        std::vector<uint8_t> one(32 * m, 0);
        for (uint32_t j = 0; j < m; ++j) one[32 * j + P[j] / 8] |= static_cast<uint8_t>(1u << (P[j] % 8));
        uint32_t neq1[256][sg::kTEditWords];
        std::fill(&neq1[0][0], &neq1[0][0] + 256 * sg::kTEditWords, 0xDEADBEEFu);
        sg::mis_neq_classes(one.data(), m, neq1);
        check(std::equal(&neq[0][0], &neq[0][0] + 256 * sg::kTEditWords, &neq1[0][0]), "mis_neq_classes of singletons", m);
        // random rows, a full row and (m > 1) an empty row: a bit in no mask, a bit in every mask
        std::vector<uint8_t> rows(32 * m);
        for (auto& b : rows) b = static_cast<uint8_t>(rnd(256));
        const uint32_t full = m - 1, empty = m > 1 ? m / 2 - (m / 2 == full) : m;
        for (uint32_t i = 0; i < 32; ++i) {
            rows[32 * full + i] = 0xFF;
            if (empty < m) rows[32 * empty + i] = 0;
        }
        sg::mis_neq_classes(rows.data(), m, neq1);
        bool ok = neq_is(neq1, m, [&](uint32_t j, uint32_t v) { return row_bit(rows, j, v); });
        for (uint32_t v = 0; v < 256; ++v) {
            ok = ok && !(neq1[v][full / 32] >> (full % 32) & 1);
            if (empty < m) ok = ok && (neq1[v][empty / 32] >> (empty % 32) & 1);
        }
        check(ok, "mis_neq_classes", m);
    }
}

// ---- the walk: 7 lengths x 8 budgets, every range of three kinds at every offset of a 3-run text --------------------------
struct Answer {
    bool hit;
    uint32_t dist;
};

// what the kernels compute: every run's lane starts fresh at edit_run_walk's first byte (a warm-up of m - 1), reads its
// masks from the table and keeps the answers of the END positions it owns.  out[e - from]: the window [e - m + 1, e].
template <int WORDS, int BITS>
void lane_answers(const std::vector<uint32_t>& table, uint32_t m, uint32_t k, const std::vector<uint8_t>& T, uint64_t from, uint64_t to,
                  std::vector<Answer>& out)
{
    const uint32_t bias = (1u << BITS) - 1u - k, top = m - 1;
    for (uint64_t c = from / sg::kTEditRun; c * sg::kTEditRun < to; ++c) {
        const sg::EditWalk w = sg::edit_run_walk(c, from, to, m - 1);
        sg::MisState<WORDS, BITS> st;
        sg::mis_fresh(st);
        for (int p = w.first; p < w.last; ++p) {
            const uint64_t at = c * sg::kTEditRun + static_cast<uint64_t>(static_cast<long long>(p));
            uint32_t nq[WORDS];
            for (int i = 0; i < WORDS; ++i) nq[i] = table.at(T.at(at) * WORDS + i);
            sg::mis_step<WORDS, BITS>(st, nq, bias);
            if (p < w.own) continue;
            Answer& a = out.at(at - from);
            a.hit = sg::mis_hit(st, top);
            a.dist = a.hit ? sg::mis_raw(st, top) - bias : ~0u;
        }
    }
}

// the same answers as the KERNELS take them (k_tmis.hip): every lane starts at mis_walk_start(m) before its run, whatever
// the range, walks the whole run a dword at a time — the bytes outside the text are the pads' zeros —, records per 32
// positions "over budget" and the planes' top bits, and keeps the ends of mis_group_mask(mis_keep_from, last).
template <int WORDS, int BITS>
void kernel_answers(const std::vector<uint32_t>& table, uint32_t m, uint32_t k, const std::vector<uint8_t>& T, uint64_t from, uint64_t to,
                    std::vector<Answer>& out)
{
    const uint32_t bias = (1u << BITS) - 1u - k, top = m - 1, tb = top & 31u;
    const long long n = static_cast<long long>(T.size());
    for (uint64_t c = from / sg::kTEditRun; c * sg::kTEditRun < to; ++c) {
        const sg::EditWalk w = sg::edit_run_walk(c, from, to, m - 1);
        const int lo = sg::mis_keep_from(w, m), hi = w.last;
        sg::MisState<WORDS, BITS> st;
        sg::mis_fresh(st);
        uint32_t over = 0, d[3] = {0, 0, 0};
        for (int j = sg::mis_walk_start(m) / 4; j < static_cast<int>(sg::kTEditRun / 4); ++j) {
            if ((j & 7) == 0) over = d[0] = d[1] = d[2] = 0;
            for (int i = 0; i < 4; ++i) {
                const long long at = static_cast<long long>(c * sg::kTEditRun) + 4 * j + i;
                const uint8_t byte = at < 0 || at >= n ? 0 : T[static_cast<size_t>(at)];
                uint32_t nq[WORDS];
                for (int x = 0; x < WORDS; ++x) nq[x] = table.at(byte * WORDS + x);
                sg::mis_step<WORDS, BITS>(st, nq, bias);
                const uint32_t bit = (4u * static_cast<uint32_t>(j) + static_cast<uint32_t>(i)) & 31u;
                over |= ((st.ov[WORDS - 1] >> tb) & 1u) << bit;
                for (int b = 0; b < BITS; ++b) d[b] |= ((st.c[b][WORDS - 1] >> tb) & 1u) << bit;
            }
            if ((j & 7) != 7 || j < 0) continue;
            const int g = j >> 3;
            const uint32_t keep = ~over & sg::mis_group_mask(lo, hi, g);
            for (int i = 0; i < 32; ++i) {
                const long long e = static_cast<long long>(c * sg::kTEditRun) + 32 * g + i;
                if (e < static_cast<long long>(from) || e >= static_cast<long long>(to)) {
                    if (keep >> i & 1u) out.at(0).dist = 0xDEADu;  // an answer kept outside the range: poisons the first entry
                    continue;
                }
                Answer& a = out.at(static_cast<size_t>(e) - from);
                a.hit = keep >> i & 1u;
                a.dist = a.hit ? ((d[0] >> i & 1u) | (d[1] >> i & 1u) << 1 | (d[2] >> i & 1u) << 2) - bias : ~0u;
            }
        }
    }
}

void lanes(const std::vector<uint8_t>& P, uint32_t k, const std::vector<uint8_t>& T, uint64_t from, uint64_t to, bool as_kernel, std::vector<Answer>& out)
{
    const uint32_t m = static_cast<uint32_t>(P.size());
    uint32_t neq[256][sg::kTEditWords];
    sg::mis_neq_bytes(P.data(), m, neq);
    const int words = sg::mis_words(m), bits = sg::mis_bits(k);
    std::vector<uint32_t> table(256 * words);
    sg::edit_peq_table(neq, static_cast<uint32_t>(words), table.data());
    out.assign(to - from, Answer{false, 0xBADu});
    if (as_kernel) {
        switch (words * 10 + bits) {
        case 11: kernel_answers<1, 1>(table, m, k, T, from, to, out); break;
        case 12: kernel_answers<1, 2>(table, m, k, T, from, to, out); break;
        case 13: kernel_answers<1, 3>(table, m, k, T, from, to, out); break;
        case 21: kernel_answers<2, 1>(table, m, k, T, from, to, out); break;
        case 22: kernel_answers<2, 2>(table, m, k, T, from, to, out); break;
        default: kernel_answers<2, 3>(table, m, k, T, from, to, out); break;
        }
        return;
    }
    switch (words * 10 + bits) {
    case 11: lane_answers<1, 1>(table, m, k, T, from, to, out); break;
    case 12: lane_answers<1, 2>(table, m, k, T, from, to, out); break;
    case 13: lane_answers<1, 3>(table, m, k, T, from, to, out); break;
    case 21: lane_answers<2, 1>(table, m, k, T, from, to, out); break;
    case 22: lane_answers<2, 2>(table, m, k, T, from, to, out); break;
    default: lane_answers<2, 3>(table, m, k, T, from, to, out); break;
    }
}

void check_walk()
{
    const uint64_t n = 3 * sg::kTEditRun;
    for (uint32_t m : kLengths)
        for (uint32_t k = 0; k < 8; ++k) {
            std::vector<uint8_t> T(n), P(m);
            for (auto& b : T) b = static_cast<uint8_t>("acgt"[rnd(4)]);
            for (auto& b : P) b = static_cast<uint8_t>("acgt"[rnd(4)]);
            if (m > 4) P[m / 2] = 'N';  // a byte the text holds only inside the planted copies' unchanged positions
            // copies of the pattern with k, k + 1, 0, k - 1, ... substitutions at distinct positions, across the runs' seams
            const uint32_t wants[5] = {k, k + 1, 0, k ? k - 1 : 0, k + 1};
            uint32_t planted = 0;
            for (uint64_t at = 10 % (n - m); at + m <= n; at += std::max<uint64_t>(m + 3, 20), ++planted) {
                std::vector<uint8_t> Q = P;
                std::vector<uint32_t> where(m);
                for (uint32_t j = 0; j < m; ++j) where[j] = j;
                for (uint32_t d = 0; d < std::min(wants[planted % 5], m); ++d) {
                    std::swap(where[d], where[d + rnd(m - d)]);
                    Q[where[d]] = Q[where[d]] == 'x' ? 'y' : 'x';
                }
                std::copy(Q.begin(), Q.end(), T.begin() + static_cast<long>(at));
            }
            // the definition's inner two loops, once: the distance of every start of the text (a range only says which starts count)
            std::vector<uint32_t> dist(n - m + 1, 0);
            for (uint64_t s = 0; s + m <= n; ++s)
                for (uint32_t j = 0; j < m; ++j) dist[s] += T[s + j] != P[j];
            bool ok = true;
            uint64_t hits = 0, near = 0, bad_from = 0, bad_to = 0, bad_e = 0;
            std::vector<Answer> got;
            for (uint64_t cut = 0; cut <= n && ok; ++cut)
                for (int kind = 0; kind < 3 && ok; ++kind) {
                    // cut by e_begin; cut by e_end; cut by both, 200 bytes apart
                    const uint64_t from = kind == 1 ? 0 : cut, to = kind == 0 ? n : kind == 1 ? cut : std::min<uint64_t>(cut + 200, n);
                    if (from >= to) continue;
                  for (int as_kernel = 0; as_kernel < 2 && ok; ++as_kernel) {  // from edit_run_walk's fresh start; as the kernels walk
                    lanes(P, k, T, from, to, as_kernel != 0, got);
                    for (uint64_t e = from; e < to && ok; ++e) {
                        // the outer loop of the definition: the window that ends at e counts when it begins at or behind `from`
                        const bool in_range = e + 1 >= from + m;
                        const uint64_t s = e + 1 - m;  // (read only when in_range)
                        const bool want = in_range && dist[s] <= k;
                        const Answer& a = got[e - from];
                        if (a.hit != want || (want && a.dist != dist[s])) { ok = false; bad_from = from; bad_to = to; bad_e = e; }
                        hits += want;
                        near += in_range && dist[s] == k + 1;
                    }
                  }
                }
            // k >= m: every window is a hit and none is a near-miss
            check(ok && hits > 0 && (near > 0 || k + 1 > m), "lanes from fresh starts against the definition", m * 10 + k, bad_from * 1000 + bad_to, bad_e);
        }
}

}  // namespace

int main()
{
    check_masks();
    check_walk();
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
