// text_editl_check.cpp — the host side of the long-pattern edit-distance calls on BYTE texts on the CPU
// (tests/test_text_editl.py builds it with AddressSanitizer and UBSan and runs it): the masks of
// smart_amd/csrc/teditl_host.hpp bit by bit, the word-major table, the run geometry against a restatement, and the walk of
// text_editl_scan / text_editl_find (k_teditl.hip) step by step — super-tiles, trips j0 .. RUN / PIECE - 1, 64 lanes in step
// with ONE number of active blocks, clipped starts, neutral votes — against a scalar column-by-column DP on the range.
// The walk takes the run, the piece and the workgroup's lanes as template parameters: the product's 512 / 128 / 256 in two
// cases, 128 / 32 / 128 in all the others, so that texts of one to three super-tiles stay small.
// Prints "<cases> cases, <failures> failures"; exit status 1 when a case failed.
#include "edit_block.hpp"
#include "teditl_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

namespace {

int g_cases = 0, g_failures = 0;

void check(bool ok, const char* what, unsigned a = 0, unsigned b = 0, unsigned c = 0, unsigned d = 0)
{
    ++g_cases;
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s (%u, %u, %u, %u)\n", what, a, b, c, d);
}

unsigned long long g_x = 88172645463325252ull;
unsigned rnd(unsigned mod)
{
    g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17;
    return static_cast<unsigned>((g_x >> 11) % mod);
}

bool accepts(const std::vector<uint8_t>& classes, size_t j, uint8_t v) { return classes[32 * j + (v >> 3)] >> (v & 7) & 1; }

std::vector<uint8_t> classes_of(const std::vector<uint8_t>& P)
{
    std::vector<uint8_t> classes(32 * P.size(), 0);
    for (size_t j = 0; j < P.size(); ++j) classes[32 * j + (P[j] >> 3)] |= static_cast<uint8_t>(1u << (P[j] & 7));
    return classes;
}

// The last row of Sellers' DP over text[from, to) for a pattern of classes (32 bytes per position): D[0][*] = 0, the column
// before `from` is D[i] = i.  out[e - from] = D[m][e].
std::vector<int> dp_scores(const std::vector<uint8_t>& classes, const std::vector<uint8_t>& text, size_t from, size_t to)
{
    const size_t m = classes.size() / 32;
    std::vector<int> col(m + 1), next(m + 1), out;
    out.reserve(to - from);
    for (size_t i = 0; i <= m; ++i) col[i] = static_cast<int>(i);
    for (size_t e = from; e < to; ++e) {
        next[0] = 0;
        for (size_t i = 1; i <= m; ++i) {
            const int sub = col[i - 1] + (accepts(classes, i - 1, text[e]) ? 0 : 1);
            next[i] = std::min(sub, std::min(col[i] + 1, next[i - 1] + 1));
        }
        col.swap(next);
        out.push_back(col[m]);
    }
    return out;
}

unsigned words_of(unsigned m) { return m <= 64 ? 2 : m <= 128 ? 4 : 8; }  // the width the launchers of k_teditl.hip choose

template <typename F>
void with_width(unsigned m, F f)
{
    if (m <= 64) f(std::integral_constant<int, 2>());
    else if (m <= 128) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 8>());
}

struct Walked {
    std::vector<int> dist;       // per end position of the range: the reported distance, -1: no report
    unsigned doubles = 0;        // end positions reported more than once
    unsigned stray = 0;          // an active lane read outside the text, or a report outside the range
    unsigned max_b = 0, shrinks = 0;
};

// text_editl_body on the CPU.  `table` is editl_peq_table's, MAXW words wide.  What lies outside the text reads as zero (the
// pads); an ACTIVE lane never reads there (stray).
template <int MAXW, uint32_t RUN, uint32_t PIECE, uint32_t LANES>
Walked kernel_walk(const std::vector<uint32_t>& table, uint32_t m, uint32_t k, bool all_blocks, const std::vector<uint8_t>& text, uint64_t e_begin,
                   uint64_t e_end)
{
    static_assert(RUN % PIECE == 0 && PIECE % 4 == 0 && LANES % 64 == 0, "the kernel's shape");
    constexpr int L = 64;
    const uint32_t mk = m + k, W = (m + 31) / 32;
    const bool cut = !all_blocks;
    Walked r;
    r.dist.assign(e_end - e_begin, -1);
    const uint64_t c0 = e_begin / RUN;
    const uint64_t ntiles = sg::editl_tile_count<RUN, LANES>(e_begin, e_end);
    const int j0 = sg::editl_first_piece<PIECE>(mk), x0 = -static_cast<int>(mk);
    for (uint64_t t = 0; t < ntiles; ++t)
        for (uint32_t wave = 0; wave < LANES / L; ++wave) {
            uint32_t pv[L][MAXW], mv[L][MAXW], B = cut ? 1u : W;
            int bot[L], first[L], last[L];
            uint64_t c[L];
            for (int l = 0; l < L; ++l) {
                c[l] = c0 + t * LANES + wave * L + l;
                const sg::EditlWalk wk = sg::editl_run_walk<RUN>(c[l], e_begin, e_end, mk);
                first[l] = wk.first;
                last[l] = wk.last;
                sg::block_fresh<MAXW>(pv[l], mv[l], B, m, bot[l]);
            }
            for (int j = j0; j < static_cast<int>(RUN / PIECE); ++j) {
                const int xj = j * static_cast<int>(PIECE), xlo = std::max(x0, xj);
                bool any = false;
                for (int l = 0; l < L; ++l) any = any || (first[l] < xj + static_cast<int>(PIECE) && last[l] > xlo);
                if (!any) continue;
                for (int x = xj + (((xlo - xj) >> 2) << 2); x < xj + static_cast<int>(PIECE); ++x) {
                    bool act[L], grow = false;
                    for (int l = 0; l < L; ++l) {
                        if (x == first[l]) sg::block_fresh<MAXW>(pv[l], mv[l], B, m, bot[l]);
                        act[l] = static_cast<uint32_t>(x - first[l]) < static_cast<uint32_t>(last[l] - first[l]);
                        grow = grow || (act[l] && sg::block_wants_grow(bot[l], k));
                    }
                    if (cut && B < W && grow) {
                        uint32_t b = B;
                        for (int l = 0; l < L; ++l) {
                            b = B;
                            sg::block_grow<MAXW>(pv[l], mv[l], b, m, bot[l]);
                        }
                        B = b;
                    }
                    for (int l = 0; l < L; ++l) {
                        const long long at = static_cast<long long>(c[l] * RUN) + x;
                        const bool inside = at >= 0 && at < static_cast<long long>(text.size());
                        if (act[l] && !inside) ++r.stray;
                        const uint8_t byte = inside ? text[static_cast<size_t>(at)] : 0;
                        bot[l] += sg::block_step<MAXW>(pv[l], mv[l], [&](int w) { return table[256 * w + byte]; }, B, m);
                    }
                    r.max_b = std::max(r.max_b, B);
                    if (cut)
                        for (;;) {
                            bool all = B > 1u;
                            for (int l = 0; l < L && all; ++l) all = !act[l] || sg::block_may_shrink(bot[l], k, B, m);
                            if (!all) break;
                            uint32_t b = B;
                            for (int l = 0; l < L; ++l) {
                                b = B;
                                sg::block_shrink<MAXW>(pv[l], mv[l], b, m, bot[l]);
                            }
                            B = b;
                            ++r.shrinks;
                        }
                    for (int l = 0; l < L; ++l) {
                        if (!(act[l] && j >= 0 && B == W && bot[l] <= static_cast<int>(k))) continue;
                        const uint64_t e = c[l] * RUN + static_cast<uint64_t>(x);
                        if (e < e_begin || e >= e_end) {
                            ++r.stray;
                            continue;
                        }
                        if (r.dist[e - e_begin] >= 0) ++r.doubles;
                        r.dist[e - e_begin] = bot[l];
                    }
                }
            }
        }
    return r;
}

// every end of the range: reported once with the DP's value where that is <= k, not reported elsewhere
bool agrees(const Walked& got, const std::vector<int>& want, uint32_t k)
{
    if (got.doubles || got.stray || got.dist.size() != want.size()) return false;
    for (size_t i = 0; i < want.size(); ++i)
        if (got.dist[i] != (want[i] <= static_cast<int>(k) ? want[i] : -1)) return false;
    return true;
}

template <int MAXW>
std::vector<uint32_t> table_of(const std::vector<uint8_t>& classes, uint32_t m)
{
    static uint32_t peq[256][sg::kTEditlWords];
    sg::editl_peq_classes(classes.data(), m, peq);
    std::vector<uint32_t> table(256 * MAXW);
    sg::editl_peq_table(peq, MAXW, table.data());
    return table;
}

const unsigned kMs[] = {1, 32, 33, 64, 65, 96, 97, 128, 129, 255, 256};
const unsigned kKs[] = {0, 1, 7, 8, 15, 16, 31};
const unsigned kAlphabets[] = {2, 4, 20, 256};

// A copy of P with about one byte in 24 dropped, one in 24 doubled and one in 24 replaced, written so that it ENDS at `end`
void plant(std::vector<uint8_t>& text, const std::vector<uint8_t>& P, size_t end, unsigned alphabet, bool edits)
{
    std::vector<uint8_t> copy;
    for (uint8_t v : P) {
        const unsigned r = edits ? rnd(24) : 9;
        if (r == 0) continue;
        copy.push_back(r == 2 ? static_cast<uint8_t>(rnd(alphabet)) : v);
        if (r == 1) copy.push_back(static_cast<uint8_t>(rnd(alphabet)));
    }
    if (copy.size() > end + 1) return;
    std::copy(copy.begin(), copy.end(), text.begin() + static_cast<long>(end + 1 - copy.size()));
}

// The scaled-down grid: runs of 128 in pieces of 32, workgroups of two waves: a super-tile of 16 KiB.  m + k reaches 287, so
// the warm-up spans up to nine pieces and the lanes of the range's first four runs start clipped.
constexpr uint32_t kRun = 128, kPiece = 32, kLanes = 128, kSuper = kRun * kLanes;

void walk_cases()
{
    unsigned turn = 0;
    for (unsigned m : kMs)
        with_width(m, [&](auto width) {
            constexpr int MAXW = decltype(width)::value;
            for (unsigned alphabet : kAlphabets)
                for (int kind = 0; kind < 2; ++kind) {
                    // one to three super-tiles' worth of runs, ragged at both ends; the range starts at byte 0, in the middle of a
                    // piece, or so late in a run that the next run begins fewer than m + k bytes behind it
                    const unsigned tiles = 1 + turn % 3, where = turn / 3 % 3;
                    ++turn;
                    const size_t size = tiles * kSuper + 700;
                    std::vector<uint8_t> text(size);
                    for (auto& v : text) v = static_cast<uint8_t>(rnd(alphabet));
                    const uint64_t e_begin = where == 0 ? 0 : where == 1 ? 3 * kRun + 17 + rnd(kPiece) : 5 * kRun + kRun - 1 - rnd(std::min(m, kRun - 1));
                    const uint64_t e_end = e_begin + (tiles - 1) * kSuper + kSuper / 2 + rnd(kSuper / 2 - 700) + 1;
                    std::vector<uint8_t> classes;
                    if (kind == 0) {  // a byte pattern cut from the text, with copies planted at the seams of runs, waves and super-tiles
                        std::vector<uint8_t> P(text.begin() + 200, text.begin() + 200 + m);
                        const uint64_t base = e_begin / kRun * kRun;
                        for (uint64_t end : {base + 2 * kRun - 1, base + 2 * kRun, base + 64 * kRun - 1, base + 64 * kRun + kPiece, base + kSuper - 1, base + kSuper,
                                             base + kSuper + kRun + 1, e_begin + m / 2, e_end - 1})
                            if (end >= e_begin + m + 40 || end == e_begin + m / 2)
                                if (end < size) plant(text, P, static_cast<size_t>(end), alphabet, end % 2 == 1);
                        classes = classes_of(P);
                    } else {          // random classes: some empty, some full, most a few values
                        classes.assign(32 * m, 0);
                        for (unsigned j = 0; j < m; ++j) {
                            const unsigned r = rnd(16);
                            if (r == 0) continue;
                            if (r == 1) {
                                std::fill(classes.begin() + 32 * j, classes.begin() + 32 * j + 32, 0xff);
                                continue;
                            }
                            for (unsigned i = 0; i < 1 + alphabet / 4; ++i) {
                                const unsigned v = rnd(alphabet);
                                classes[32 * j + (v >> 3)] |= static_cast<uint8_t>(1u << (v & 7));
                            }
                        }
                    }
                    const std::vector<uint32_t> table = table_of<MAXW>(classes, m);
                    const std::vector<int> want = dp_scores(classes, text, e_begin, e_end);
                    for (unsigned k : kKs) {
                        check(agrees(kernel_walk<MAXW, kRun, kPiece, kLanes>(table, m, k, false, text, e_begin, e_end), want, k), "the walk with the cut-off", m,
                              alphabet, kind, k);
                        check(agrees(kernel_walk<MAXW, kRun, kPiece, kLanes>(table, m, k, true, text, e_begin, e_end), want, k), "the walk with all blocks", m,
                              alphabet, kind, k);
                    }
                }
            // planted prefixes of the pattern, each followed by a byte the next position does not accept: blocks switch on and off
            for (unsigned k : {0u, 7u, 31u}) {
                // B is the WAVE's, and a block is dropped only when all 64 lanes agree.  So: all 256 values (on four, the lanes of a
                // wave never agree that a full block of random text is beyond k), ONE prefix per wave (64 runs), ending at byte 60 of
                // a run in the wave's middle: the lane that owns its end walks 67 bytes of noise behind it before the runs end.
                std::vector<unsigned> lens;
                for (unsigned len : {31u, 32u, 33u, 64u, 100u, 200u, m - 1})
                    if (len != 0 && len < m) lens.push_back(len);
                std::vector<uint8_t> P(m), text(std::max<size_t>(lens.size(), 1) * 64 * kRun + 300);
                for (auto& v : P) v = static_cast<uint8_t>(rnd(256));
                for (auto& v : text) v = static_cast<uint8_t>(rnd(256));
                unsigned longest = 0;
                for (size_t i = 0; i < lens.size(); ++i) {
                    const unsigned len = lens[i];
                    const size_t end = (64 * i + 30) * kRun + 60;  // the prefix's last byte
                    std::copy(P.begin(), P.begin() + len, text.begin() + static_cast<long>(end + 1 - len));
                    text[end + 1] = static_cast<uint8_t>(P[len] + 1);
                    longest = std::max(longest, len);
                }
                const std::vector<uint8_t> classes = classes_of(P);
                const std::vector<uint32_t> table = table_of<MAXW>(classes, m);
                const std::vector<int> want = dp_scores(classes, text, 0, text.size());
                const Walked got = kernel_walk<MAXW, kRun, kPiece, kLanes>(table, m, k, false, text, 0, text.size());
                // a prefix of 32 bytes or more of a pattern of more than one block switches the second block on; at a small k the
                // random text behind it switches it off again (at k = 31 a block of random text stays below k + 32: no claim)
                const bool switched = (m + 31) / 32 < 2 || longest < 32 || (got.max_b >= 2 && (k > 7 || got.shrinks >= 1));
                check(agrees(got, want, k) && switched, "planted prefixes", m, k, got.max_b, got.shrinks);
            }
        });
}

// the product's own geometry, once per width's end: runs of 512 in pieces of 128, 256 lanes, a super-tile and a ragged one
void product_cases()
{
    for (unsigned m : {100u, 256u})
        with_width(m, [&](auto width) {
            constexpr int MAXW = decltype(width)::value;
            const unsigned k = m == 100 ? 7 : 31;
            std::vector<uint8_t> text(sg::kTEditlSuper + 5 * sg::kTEditlRun + 77);
            for (auto& v : text) v = static_cast<uint8_t>(rnd(4));
            const std::vector<uint8_t> P(text.begin() + 1000, text.begin() + 1000 + m);
            const uint64_t e_begin = m == 100 ? 0 : 300, e_end = text.size() - (m == 100 ? 0 : 40);
            for (uint64_t end : {uint64_t(sg::kTEditlRun - 1), uint64_t(sg::kTEditlRun), uint64_t(64 * sg::kTEditlRun), uint64_t(sg::kTEditlSuper - 1),
                                 uint64_t(sg::kTEditlSuper), uint64_t(sg::kTEditlSuper + sg::kTEditlRun + 3)})
                plant(text, P, static_cast<size_t>(end), 4, end % 2 == 1);
            const std::vector<uint8_t> classes = classes_of(P);
            const std::vector<uint32_t> table = table_of<MAXW>(classes, m);
            check(agrees(kernel_walk<MAXW, sg::kTEditlRun, sg::kTEditlPiece, sg::kTEditlLanes>(table, m, k, false, text, e_begin, e_end),
                         dp_scores(classes, text, e_begin, e_end), k),
                  "the product's geometry", m, k);
        });
}

// editl_run_walk against a restatement: the owned positions are the run's inside the range, the walk starts mk bytes before
// the first of them or at e_begin, whichever is later
template <uint32_t RUN>
bool run_walk_restated()
{
    bool ok = true;
    for (int i = 0; i < 4000; ++i) {
        const uint64_t e_begin = rnd(3) ? rnd(6 * RUN) : 0, e_end = e_begin + rnd(5 * RUN);
        const uint32_t mk = 1 + rnd(287);
        const uint64_t c = rnd(13);
        const sg::EditlWalk w = sg::editl_run_walk<RUN>(c, e_begin, e_end, mk);
        long long lo = -1, hi = -1;
        for (uint64_t e = c * RUN; e < (c + 1) * RUN; ++e)
            if (e >= e_begin && e < e_end) {
                if (lo < 0) lo = static_cast<long long>(e);
                hi = static_cast<long long>(e) + 1;
            }
        const long long base = static_cast<long long>(c * RUN);
        if (lo < 0) {
            ok = ok && w.first == 0 && w.own == 0 && w.last == 0;
        } else {
            const long long start = std::max<long long>(static_cast<long long>(e_begin), lo - static_cast<long long>(mk));
            ok = ok && w.first == start - base && w.own == lo - base && w.last == hi - base && w.own == std::max(w.first, 0) && w.first >= -static_cast<int>(mk);
        }
    }
    return ok;
}

// editl_tile_count: the smallest number of super-tiles, from the run that holds e_begin on, that covers the range
template <uint32_t RUN, uint32_t LANES>
bool tile_count_restated()
{
    bool ok = true;
    for (int i = 0; i < 4000; ++i) {
        const uint64_t e_begin = rnd(3) ? rnd(3 * RUN * LANES) : 0, e_end = e_begin + 1 + rnd(3 * RUN * LANES);
        const uint64_t start = e_begin - e_begin % RUN;
        uint64_t tiles = 0;
        while (start + tiles * RUN * LANES < e_end) ++tiles;
        ok = ok && sg::editl_tile_count<RUN, LANES>(e_begin, e_end) == tiles;
    }
    return ok;
}

void geometry_cases()
{
    check(run_walk_restated<sg::kTEditlRun>(), "editl_run_walk, runs of 512");
    check(run_walk_restated<kRun>(), "editl_run_walk, runs of 128");
    check(tile_count_restated<sg::kTEditlRun, sg::kTEditlLanes>(), "editl_tile_count, the product's super-tile");
    check(tile_count_restated<kRun, kLanes>(), "editl_tile_count, the scaled super-tile");
    bool ok = true;
    for (uint32_t mk = 1; mk <= 287; ++mk) {
        int j = 0;
        while (j * static_cast<int>(sg::kTEditlPiece) > -static_cast<int>(mk)) --j;  // the last j with 128 j <= -mk
        ok = ok && sg::editl_first_piece(mk) == j && j >= -3;
    }
    check(ok, "editl_first_piece");
}

void peq_cases()
{
    static uint32_t peq[256][sg::kTEditlWords];
    for (unsigned alphabet : kAlphabets)
        for (unsigned m : {1u, 33u, 255u, 256u}) {
            std::vector<uint8_t> P(m);
            for (auto& v : P) v = static_cast<uint8_t>(rnd(alphabet));
            sg::editl_peq_bytes(P.data(), m, peq);
            bool ok = true;
            for (unsigned j = 0; j < 32 * sg::kTEditlWords; ++j)
                for (unsigned v = 0; v < 256; ++v) ok = ok && (peq[v][j >> 5] >> (j & 31) & 1) == (j < m && P[j] == v);
            check(ok, "editl_peq_bytes", alphabet, m);
            std::vector<uint8_t> classes(32 * m);
            for (unsigned j = 0; j < m; ++j)
                for (unsigned i = 0; i < 32; ++i) classes[32 * j + i] = j % 4 == 0 ? 0 : j % 4 == 1 ? 0xff : static_cast<uint8_t>(rnd(256));
            sg::editl_peq_classes(classes.data(), m, peq);
            ok = true;
            for (unsigned j = 0; j < 32 * sg::kTEditlWords; ++j)
                for (unsigned v = 0; v < 256; ++v) ok = ok && (peq[v][j >> 5] >> (j & 31) & 1) == (j < m && accepts(classes, j, static_cast<uint8_t>(v)));
            check(ok, "editl_peq_classes", alphabet, m);
            // the table: WORD-major, words dwords per value, nothing written behind 256 * words
            const unsigned words = words_of(m);
            std::vector<uint32_t> table(256 * words + 1, 0xdeadbeefu);
            sg::editl_peq_table(peq, words, table.data());
            ok = table[256 * words] == 0xdeadbeefu;
            for (unsigned w = 0; w < words; ++w)
                for (unsigned v = 0; v < 256; ++v) ok = ok && table[w * 256 + v] == peq[v][w];
            check(ok, "editl_peq_table", alphabet, m);
        }
}

}  // namespace

int main()
{
    peq_cases();
    geometry_cases();
    walk_cases();
    product_cases();
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
