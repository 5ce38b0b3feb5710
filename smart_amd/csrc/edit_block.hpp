// edit_block.hpp — one column of the edit-distance search for LONG patterns (smartgpu_psearch_editl64, peditl.hpp): the
// recurrence of edit_step.hpp — Myers' bit-vector recurrence in Hyyrö's search form — in BLOCKS of 32 rows, of which only
// the first B are computed (Ukkonen's cut-off).  Host and device: planes_editl_scan / planes_editl_find (k_peditl.hip)
// run it per text symbol and lane, tests/packed_editl_check.cpp runs it on the CPU against the plain DP.
// No HIP call, no other header of the library.
//
// The pattern's m rows lie in W = ceil(m / 32) blocks; block w holds rows 32 w + 1 .. 32 w + rows(w), its vertical
// differences in pv[w] / mv[w] as edit_step.hpp holds them.  The ACTIVE blocks are 0 .. B - 1, 1 <= B <= W; `bot` is the
// value D at the bottom row of block B - 1, the only score that is kept: the bottom of the block above it is bot less the
// vertical differences of block B - 1 (two population counts, taken when a block is dropped), so no score per block is
// carried.  Stepping blocks 0 .. B - 1 as one multi-word integer IS the recurrence on the pattern's first 32 B symbols:
// the addition's carry and the shifted-in bits of Ph / Mh run from dword to dword in one forward pass.
//
// The cut-off, per column (k the budget):
//   grow    before a symbol is consumed, if B < W and bot <= k: block B becomes active as a FRESH one (Pv all ones, Mv
//           zero, bot += rows(B)) — an upper bound of the true values, as the column D[i] = i of edit_step.hpp is;
//   step    blocks 0 .. B - 1, bot follows bit rows(B - 1) - 1 of the last one's Ph / Mh;
//   shrink  while B > 1 and bot >= k + rows(B - 1), block B - 1 is dropped: its values differ by at most one from row to
//           row, so every one of them is > k;
//   report  the column's end is an occurrence iff B == W and bot <= k.
// Why the values <= k are exact: values along a DP path never decrease, so a cell <= k derives only from cells <= k, and
// those lie in active blocks (a block is inactive only while all its cells, and the row above it, are > k); everything that
// is computed is >= the true value (a fresh block is an upper bound and the recurrence is monotone in its left column).
// Hence every computed value <= k is the true one, and whatever is > k or not computed is truly > k.  A caller may carry
// MORE blocks than this rule asks for — grow early, shrink late — by the same argument: k_peditl.hip keeps B equal across
// a wave.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SG_BLOCK_HD __host__ __device__ __forceinline__
#define SG_BLOCK_UNROLL _Pragma("unroll")   // every loop over blocks: the device indexes pv / mv by constants only
#else
#define SG_BLOCK_HD inline
#define SG_BLOCK_UNROLL
#endif

namespace sg {

// rows of block w of a pattern of m symbols (w < ceil(m / 32))
SG_BLOCK_HD uint32_t block_rows(uint32_t m, uint32_t w) { return m - 32u * w < 32u ? m - 32u * w : 32u; }

// The column before which nothing was read, D[i] = i, on B active blocks: bot = min(32 B, m).
template <int MAXW>
SG_BLOCK_HD void block_fresh(uint32_t (&pv)[MAXW], uint32_t (&mv)[MAXW], uint32_t B, uint32_t m, int& bot)
{
    SG_BLOCK_UNROLL
    for (int w = 0; w < MAXW; ++w) {
        pv[w] = ~0u;
        mv[w] = 0u;
    }
    bot = static_cast<int>(32u * B < m ? 32u * B : m);
}

SG_BLOCK_HD bool block_wants_grow(int bot, uint32_t k) { return bot <= static_cast<int>(k); }
SG_BLOCK_HD bool block_may_shrink(int bot, uint32_t k, uint32_t B, uint32_t m) { return bot >= static_cast<int>(k + block_rows(m, B - 1)); }

// Block B (B < ceil(m / 32) <= MAXW) becomes active.  (Comparisons with w, not pv[B]: the device keeps the arrays in registers.)
template <int MAXW>
SG_BLOCK_HD void block_grow(uint32_t (&pv)[MAXW], uint32_t (&mv)[MAXW], uint32_t& B, uint32_t m, int& bot)
{
    SG_BLOCK_UNROLL
    for (int w = 1; w < MAXW; ++w)
        if (static_cast<uint32_t>(w) == B) {
            pv[w] = ~0u;
            mv[w] = 0u;
        }
    bot += static_cast<int>(block_rows(m, B));
    ++B;
}

// Block B - 1 (B > 1) is dropped: bot becomes the value at the bottom row of block B - 2.
template <int MAXW>
SG_BLOCK_HD void block_shrink(const uint32_t (&pv)[MAXW], const uint32_t (&mv)[MAXW], uint32_t& B, uint32_t m, int& bot)
{
    uint32_t p = 0u, n = 0u;
    SG_BLOCK_UNROLL
    for (int w = 1; w < MAXW; ++w)
        if (static_cast<uint32_t>(w) == B - 1u) {
            p = pv[w];
            n = mv[w];
        }
    const uint32_t rows = block_rows(m, B - 1u), mask = rows == 32u ? ~0u : (1u << rows) - 1u;
    bot += __builtin_popcount(n & mask) - __builtin_popcount(p & mask);
    --B;
}

// One text symbol through Eq (bit j of dword j / 32: pattern position j accepts it; zero beyond m) on blocks 0 .. B - 1.
// eq_of(w) gives dword w of Eq, w a constant after unrolling; it is asked for the active blocks only, so that an inactive
// block costs the device nothing but the branch over it.  Returns the change of bot.  Bits from m on, in the last block,
// hold what the additions carry into them; nothing below depends on them.
template <int MAXW, typename EqOf>
SG_BLOCK_HD int block_step(uint32_t (&pv)[MAXW], uint32_t (&mv)[MAXW], EqOf&& eq_of, uint32_t B, uint32_t m)
{
    const uint32_t top = m - 1u;
    uint32_t carry = 0u, hp = 0u, hm = 0u;  // (the SEARCH form: row 0 is all zeros, no 1 enters the shifted Ph of block 0)
    int delta = 0;
    SG_BLOCK_UNROLL
    for (int w = 0; w < MAXW; ++w) {
        if (static_cast<uint32_t>(w) >= B) continue;  // (a predicate per unrolled block, never an index under a run-time bound)
        const uint32_t eq = eq_of(w);
        const uint32_t x = eq & pv[w];
        const uint32_t s1 = x + pv[w];     // (Eq & Pv) + Pv over the B dwords: the carry runs from dword to dword
        const uint32_t s = s1 + carry;
        carry = static_cast<uint32_t>(s1 < x) | static_cast<uint32_t>(s < s1);
        const uint32_t xh = (s ^ pv[w]) | eq;
        const uint32_t xv = eq | mv[w];
        uint32_t ph = mv[w] | ~(xh | pv[w]);
        uint32_t mh = pv[w] & xh;
        if (static_cast<uint32_t>(w) == B - 1u) {
            const uint32_t bit = static_cast<uint32_t>(w) == top >> 5 ? top & 31u : 31u;
            delta = static_cast<int>((ph >> bit) & 1u) - static_cast<int>((mh >> bit) & 1u);
        }
        const uint32_t php = ph >> 31, mhp = mh >> 31;
        ph = ph << 1 | hp;
        mh = mh << 1 | hm;
        hp = php;
        hm = mhp;
        pv[w] = mh | ~(xv | ph);
        mv[w] = ph & xv;
    }
    return delta;
}

}  // namespace sg
