// tmis_host.hpp — byte texts: what the mismatch calls of match_calls.cpp (smartgpu_search_mis64 and its kin) decide on the host
// before a launch, and the recurrence the kernels of k_tmis.hip run per text byte and lane.  The pattern becomes 256 masks,
// one per byte value — tedit_host.hpp's, complemented below m —; a lane's run becomes three numbers (edit_run_walk with a
// warm-up of m - 1 bytes); a window's mismatches are counted in bit-sliced counters that move with the text.  Host and
// device, no HIP call, no error text — tests/text_mis_check.cpp runs all of it without a device.
//
// THE RECURRENCE is planes_mis_scan's counter (k_planes.hip) turned so that a lane walks the text: there bit i of a dword
// is start position i and the loop runs over the pattern; here bit j is the window that started j bytes ago and the loop
// runs over the text.  The state is BITS counter planes c[b] and a sticky plane ov, WORDS dwords each.  After the step for
// text byte i, bit j describes the window that started at byte i - j: the planes hold the number of its mismatches so far
// plus BIAS = 2^BITS - 1 - k, ov says that the biased count has overflowed — more than k mismatches.  A fresh start is
// c[b] = 0, ov = all ones: a window that began before the first walked byte can never be a hit, which is also the clip at
// the range's first byte.  Per byte v:
//     c[b] = c[b] << 1 | bit b of BIAS;  ov = ov << 1          a new window enters at bit 0 (the shift carries across dwords)
//     carry = neq[v]                                            bit j: pattern position j does NOT accept v
//     t = c[0] & carry;  c[0] ^= carry;  carry = t;  ... c[1], c[2] ...;  ov |= carry
// and the window that ENDS at this byte, start s = i - m + 1, is an occurrence when bit m - 1 of ov is clear; its distance
// is the value of bits m - 1 of c[BITS-1 .. 0] minus BIAS.  Nothing is masked to m bits: bits at or above m are never read
// and never move downward (shifts go up, the adder works within a bit position).  A Hamming window needs exactly its own m
// bytes, so a lane that starts fresh m - 1 bytes before its first owned END position is exact with nothing to prove.
#pragma once
#include "tedit_host.hpp"

namespace sg {

constexpr uint32_t kTMisMaxM = 64;  // SMARTGPU_MIS_MAXM
static_assert(kTMisMaxM == kTEditMaxM, "the masks are tedit_host.hpp's: kTEditWords dwords");
static_assert(kTEditRun >= kTMisMaxM - 1, "the warm-up of the longest pattern lies in the neighbour's run");

// neq[v][j / 32] bit j % 32 = pattern position j does NOT accept byte v; zero from m on.  A byte the pattern does not hold
// has all m bits: a mismatch at every position, which is all the recurrence needs to know of it.
inline void mis_complement(uint32_t m, uint32_t (&neq)[256][kTEditWords])
{
    for (uint32_t v = 0; v < 256; ++v)
        for (uint32_t w = 0; w < kTEditWords; ++w) {
            const uint32_t below = m >= 32 * (w + 1) ? ~0u : m > 32 * w ? (1u << (m - 32 * w)) - 1u : 0u;
            neq[v][w] = ~neq[v][w] & below;
        }
}
inline void mis_neq_bytes(const uint8_t* P, uint32_t m, uint32_t (&neq)[256][kTEditWords])
{
    edit_peq_bytes(P, m, neq);
    mis_complement(m, neq);
}
// The same from classes (edit_peq_classes' rows): an empty row has its bit in every mask, a full row in none.
inline void mis_neq_classes(const uint8_t* classes, uint32_t m, uint32_t (&neq)[256][kTEditWords])
{
    edit_peq_classes(classes, m, neq);
    mis_complement(m, neq);
}
// (the masks as the kernels read them: edit_peq_table, WORDS dwords per byte value)

constexpr int mis_words(uint32_t m) { return m <= 32 ? 1 : 2; }
constexpr int mis_bits(uint32_t k) { return k <= 1 ? 1 : k <= 3 ? 2 : 3; }

// THE WALK of the kernels.  edit_run_walk(c, e_begin, e_end, m - 1) says which bytes decide a lane's owned ends: [first,
// last) relative to the run, first = max(own - (m - 1), e_begin).  Walking MORE bytes before `first` changes nothing for a
// window that lies behind them, so the kernels start every lane of a workgroup at the same dword, mis_walk_start(m) bytes
// before the run — a scalar loop counter, whole dwords, no edge cases — and walk the whole run.  What e_begin clips is then
// decided where an answer is kept, not by the fresh start: of the ends [own, last) a lane keeps those whose window begins
// at or behind `first`, [mis_keep_from(w, m), last).  (For first = own - (m - 1) that is every owned end.)
SG_HOST_DEVICE inline int mis_walk_start(uint32_t m) { return -static_cast<int>((m - 1 + 3) / 4 * 4); }
SG_HOST_DEVICE inline int mis_keep_from(const EditWalk& w, uint32_t m)
{
    const int from = w.first + static_cast<int>(m - 1);
    return from > w.own ? (from < w.last ? from : w.last) : w.own;
}
// bits [lo, hi) of the 32 positions [32 g, 32 g + 32) of a run
SG_HOST_DEVICE inline uint32_t mis_group_mask(int lo, int hi, int g)
{
    const int a = lo - 32 * g, b = hi - 32 * g;
    const uint32_t below_b = b <= 0 ? 0u : b >= 32 ? ~0u : (1u << b) - 1u;
    const uint32_t below_a = a <= 0 ? 0u : a >= 32 ? ~0u : (1u << a) - 1u;
    return below_b & ~below_a;
}

template <int WORDS, int BITS>
struct MisState {
    uint32_t c[BITS][WORDS], ov[WORDS];
};

template <int WORDS, int BITS>
SG_HOST_DEVICE inline void mis_fresh(MisState<WORDS, BITS>& s)
{
    for (int w = 0; w < WORDS; ++w) {
        for (int b = 0; b < BITS; ++b) s.c[b][w] = 0u;
        s.ov[w] = ~0u;
    }
}

// One text byte, through its mask.  bias = 2^BITS - 1 - k (k < 2^BITS).
template <int WORDS, int BITS>
SG_HOST_DEVICE inline void mis_step(MisState<WORDS, BITS>& s, const uint32_t (&neq)[WORDS], uint32_t bias)
{
    static_assert(WORDS == 1 || WORDS == 2, "one dword for m <= 32, two for m <= 64");
    static_assert(BITS >= 1 && BITS <= 3, "budgets up to 1 / 3 / 7");
    for (int b = 0; b < BITS; ++b) {
        for (int w = WORDS - 1; w > 0; --w) s.c[b][w] = s.c[b][w] << 1 | s.c[b][w - 1] >> 31;
        s.c[b][0] = s.c[b][0] << 1 | ((bias >> b) & 1u);
    }
    for (int w = WORDS - 1; w > 0; --w) s.ov[w] = s.ov[w] << 1 | s.ov[w - 1] >> 31;
    s.ov[0] <<= 1;
    for (int w = 0; w < WORDS; ++w) {
        uint32_t carry = neq[w];
        for (int b = 0; b < BITS; ++b) {
            const uint32_t t = s.c[b][w] & carry;
            s.c[b][w] ^= carry;
            carry = t;
        }
        s.ov[w] |= carry;
    }
}

// The window that ends at the byte just stepped.  top = m - 1, which lies in the LAST dword: 32 (WORDS - 1) <= top < 32 WORDS
// (mis_words).  mis_hit: at most k mismatches; mis_raw: the biased count, the distance is mis_raw - bias (a hit's only).
template <int WORDS, int BITS>
SG_HOST_DEVICE inline bool mis_hit(const MisState<WORDS, BITS>& s, uint32_t top)
{
    return !((s.ov[WORDS - 1] >> (top & 31u)) & 1u);
}
template <int WORDS, int BITS>
SG_HOST_DEVICE inline uint32_t mis_raw(const MisState<WORDS, BITS>& s, uint32_t top)
{
    uint32_t v = 0;
    for (int b = 0; b < BITS; ++b) v |= ((s.c[b][WORDS - 1] >> (top & 31u)) & 1u) << b;
    return v;
}

}  // namespace sg
