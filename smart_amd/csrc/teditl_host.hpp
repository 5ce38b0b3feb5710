// teditl_host.hpp — byte texts, LONG patterns: what the calls of match_calls.cpp (smartgpu_search_editl64 and its kin) decide on the
// host before a launch, and the geometry the kernels of k_teditl.hip share with it.  The pattern becomes 256 masks of up to
// eight dwords, which the block recurrence of edit_block.hpp consumes one dword per active block; a lane's run becomes three
// numbers; a range becomes a number of super-tiles.  No HIP call, no error text — tests/text_editl_check.cpp runs all of it
// without a device, and walks the kernels' trips on the CPU with the same functions.
#pragma once
#include "edit_block.hpp"

#include <cstring>

namespace sg {

constexpr uint32_t kTEditlMaxM = 256;                    // SMARTGPU_EDITL_MAXM
constexpr uint32_t kTEditlMaxK = 31;                     // SMARTGPU_EDITL_MAXK
constexpr uint32_t kTEditlWords = 8;                     // dwords of one mask
static_assert(kTEditlWords * 32 == kTEditlMaxM, "a mask holds the longest pattern");

// peq[v][j / 32] bit j % 32 = pattern position j accepts byte v; zero beyond m (edit_peq_bytes' rules, tedit_host.hpp: a
// byte the pattern does not hold has an all-zero mask).
inline void editl_peq_bytes(const uint8_t* P, uint32_t m, uint32_t (&peq)[256][kTEditlWords])
{
    std::memset(peq, 0, sizeof peq);
    for (uint32_t j = 0; j < m; ++j) peq[P[j]][j >> 5] |= 1u << (j & 31);
}

// The same from classes (edit_peq_classes' rules): classes[32 * j + v / 8] bit v % 8 = position j accepts byte v.  An empty
// row has no bit anywhere, a full row one in every mask.
inline void editl_peq_classes(const uint8_t* classes, uint32_t m, uint32_t (&peq)[256][kTEditlWords])
{
    std::memset(peq, 0, sizeof peq);
    for (uint32_t j = 0; j < m; ++j)
        for (uint32_t v = 0; v < 256; ++v)
            if (classes[32 * j + (v >> 3)] >> (v & 7) & 1u) peq[v][j >> 5] |= 1u << (j & 31);
}

// The masks as the kernels read them, WORD-MAJOR: table[w * 256 + v], 256 * words dwords (words = 2, 4, 8).  A step reads
// one dword per ACTIVE block, each with its own ds_read_b32: dword w of byte v lies on bank v mod 32 whatever w is, as in
// tedit_host.hpp's one-dword table.  (Byte-major, eight dwords per value, would put all 256 values on four banks.)
inline void editl_peq_table(const uint32_t (&peq)[256][kTEditlWords], uint32_t words, uint32_t* table)
{
    for (uint32_t w = 0; w < words; ++w)
        for (uint32_t v = 0; v < 256; ++v) table[w * 256 + v] = peq[v][w];
}

// THE GEOMETRY (k_teditl.hip says why).  A lane owns kTEditlRun consecutive END positions and walks them in pieces of
// kTEditlPiece bytes; the kTEditlLanes lanes of a workgroup own a SUPER-TILE.  The functions below take the three numbers
// as template parameters so that tests/text_editl_check.cpp can walk a scaled-down grid; the kernels use the defaults.
constexpr uint32_t kTEditlRun = 512;
constexpr uint32_t kTEditlPiece = 128;
constexpr uint32_t kTEditlLanes = 256;
constexpr uint32_t kTEditlSuper = kTEditlLanes * kTEditlRun;   // bytes of text a workgroup owns per super-tile

// Which bytes the lane of run c (end positions [RUN c, RUN c + RUN)) walks, relative to the run's first byte, for the range
// [e_begin, e_end) and a warm-up of mk = m + k bytes — edit_run_walk (tedit_host.hpp) on the longer run: it starts fresh
// at `first`, walks [first, last) one byte per step and counts only from `own` = max(first, 0) on.  The bytes below 0 are the
// warm-up, at most mk of them; a run that e_begin cuts, or that begins fewer than mk bytes behind e_begin, starts AT e_begin,
// which is the definition and no warm-up.  A run outside the range is first = own = last = 0: nothing walked.
struct EditlWalk {
    int first, own, last;
};
template <uint32_t RUN = kTEditlRun>
SG_BLOCK_HD EditlWalk editl_run_walk(uint64_t c, uint64_t e_begin, uint64_t e_end, uint32_t mk)
{
    const uint64_t base = c * RUN;
    const uint64_t own_lo = base > e_begin ? base : e_begin, own_hi = base + RUN < e_end ? base + RUN : e_end;
    EditlWalk w = {0, 0, 0};
    if (own_lo >= own_hi) return w;
    const uint64_t start = own_lo - e_begin > mk ? own_lo - mk : e_begin;
    w.first = static_cast<int>(static_cast<long long>(start - base));
    w.own = static_cast<int>(own_lo - base);
    w.last = static_cast<int>(own_hi - base);
    return w;
}

// The super-tiles of [e_begin, e_end): the first begins at the run that holds e_begin.  The kernels' trip count AND the
// host's grid (text_tile_count's role): the same for every lane of the grid.
template <uint32_t RUN = kTEditlRun, uint32_t LANES = kTEditlLanes>
SG_BLOCK_HD uint64_t editl_tile_count(uint64_t e_begin, uint64_t e_end)
{
    return (e_end - e_begin / RUN * RUN + uint64_t(LANES) * RUN - 1) / (uint64_t(LANES) * RUN);
}

// The first piece of a super-tile's walk: pieces j0 .. -1 hold the warm-up (the neighbour run's last pieces), pieces
// 0 .. RUN / PIECE - 1 the owned positions.  A function of the kernel arguments only.
template <uint32_t PIECE = kTEditlPiece>
SG_BLOCK_HD int editl_first_piece(uint32_t mk)
{
    return -static_cast<int>((mk + PIECE - 1) / PIECE);
}

}  // namespace sg
