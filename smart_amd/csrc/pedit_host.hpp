// pedit_host.hpp — what the edit-distance calls of match_calls.cpp decide on the host before a launch: the pattern as the masks
// Peq the recurrence of edit_step.hpp consumes.  Host only: no HIP call, no error text — tests/packed_edit_check.cpp runs
// it without a device.
#pragma once
#include "edit_step.hpp"

#include <cstring>

namespace sg {

constexpr uint32_t kEditMaxM = 64;                    // SMARTGPU_PEDIT_MAXM
constexpr uint32_t kEditWords = kEditMaxM / 32;       // dwords of one mask

// peq[c][j / 32] bit j % 32 = pattern position j accepts code c (the rank of a byte value among the text's `values`,
// ascending, nvalues of them); zero beyond m and for the codes the text does not hold.  A byte the text does not hold
// has its bit in NO mask: it matches nothing, which is all the recurrence needs to know of it.
inline void edit_peq_pattern(const uint8_t values[4], int nvalues, const uint8_t* P, uint32_t m, uint32_t (&peq)[4][kEditWords])
{
    std::memset(peq, 0, sizeof peq);
    for (uint32_t j = 0; j < m; ++j)
        for (int c = 0; c < nvalues; ++c)
            if (values[c] == P[j]) peq[c][j >> 5] |= 1u << (j & 31);
}

// The same from sets: bit c of sets[j] = position j accepts code c.  An empty set has no bit anywhere, a full set one in
// the mask of every code the text holds.  Returns -1, or the first position whose set names a code >= nvalues (peq is
// then unfinished).
inline int edit_peq_sets(int nvalues, const uint8_t* sets, uint32_t m, uint32_t (&peq)[4][kEditWords])
{
    const uint32_t all = (1u << nvalues) - 1u;
    std::memset(peq, 0, sizeof peq);
    for (uint32_t j = 0; j < m; ++j) {
        if (sets[j] & ~all) return static_cast<int>(j);
        for (uint32_t c = 0; c < 4; ++c)
            if (sets[j] >> c & 1u) peq[c][j >> 5] |= 1u << (j & 31);
    }
    return -1;
}

}  // namespace sg
