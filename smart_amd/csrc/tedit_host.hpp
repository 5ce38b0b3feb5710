// tedit_host.hpp — byte texts: what the edit-distance calls of match_calls.cpp (smartgpu_search_edit64 and its kin) decide on the
// host before a launch, and the run geometry the kernels of k_tedit.hip share with it.  The pattern becomes 256 masks, one
// per byte value, which the recurrence of edit_step.hpp consumes; a lane's run becomes three numbers.  No HIP call, no
// error text — tests/text_edit_check.cpp runs all of it without a device.
#pragma once
#include "edit_step.hpp"

#include <cstring>

namespace sg {

constexpr uint32_t kTEditMaxM = 64;                    // SMARTGPU_EDIT_MAXM
constexpr uint32_t kTEditWords = kTEditMaxM / 32;      // dwords of one mask
constexpr uint32_t kTEditRun = 128;                    // end positions a lane owns: pedit.hpp's kEditRun, a wave covers kFindSpan

// peq[v][j / 32] bit j % 32 = pattern position j accepts byte v; zero beyond m.  A byte the pattern does not hold has an
// all-zero mask: it matches nothing, which is all the recurrence needs to know of it.
inline void edit_peq_bytes(const uint8_t* P, uint32_t m, uint32_t (&peq)[256][kTEditWords])
{
    std::memset(peq, 0, sizeof peq);
    for (uint32_t j = 0; j < m; ++j) peq[P[j]][j >> 5] |= 1u << (j & 31);
}

// The same from classes: classes[32 * j + v / 8] bit v % 8 = position j accepts byte v (a 256-bit row per position).  An
// empty row has no bit anywhere, a full row one in every mask.
inline void edit_peq_classes(const uint8_t* classes, uint32_t m, uint32_t (&peq)[256][kTEditWords])
{
    std::memset(peq, 0, sizeof peq);
    for (uint32_t j = 0; j < m; ++j)
        for (uint32_t v = 0; v < 256; ++v)
            if (classes[32 * j + (v >> 3)] >> (v & 7) & 1u) peq[v][j >> 5] |= 1u << (j & 31);
}

// The masks as the kernels read them: WORDS dwords per byte value, 256 * WORDS dwords in all (WORDS = 1: m <= 32).
inline void edit_peq_table(const uint32_t (&peq)[256][kTEditWords], uint32_t words, uint32_t* table)
{
    for (uint32_t v = 0; v < 256; ++v)
        for (uint32_t w = 0; w < words; ++w) table[v * words + w] = peq[v][w];
}

// Which bytes the lane of run c (end positions [128 c, 128 c + 128)) walks, relative to the run's first byte, for the
// range [e_begin, e_end) and a warm-up of mk = m + k bytes: it starts fresh at `first`, walks [first, last) one byte per
// step and counts only from `own` on.  own = max(first, 0): the bytes below 0 are the warm-up (at most mk of them, the
// neighbour run's last bytes), and a run that e_begin cuts starts AT e_begin, which is the definition and no warm-up.
// A run outside the range is first = own = last = 0: nothing walked.
struct EditWalk {
    int first, own, last;
};
SG_HOST_DEVICE inline EditWalk edit_run_walk(uint64_t c, uint64_t e_begin, uint64_t e_end, uint32_t mk)
{
    const uint64_t base = c * kTEditRun;
    const uint64_t own_lo = base > e_begin ? base : e_begin, own_hi = base + kTEditRun < e_end ? base + kTEditRun : e_end;
    EditWalk w = {0, 0, 0};
    if (own_lo >= own_hi) return w;
    const uint64_t start = own_lo - e_begin > mk ? own_lo - mk : e_begin;
    w.first = static_cast<int>(static_cast<long long>(start - base));
    w.own = static_cast<int>(own_lo - base);
    w.last = static_cast<int>(own_hi - base);
    return w;
}

}  // namespace sg
